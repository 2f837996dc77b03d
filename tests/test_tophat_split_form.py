"""The host's rule for the split-band form of the batch top-hat walks (csrc/k_tophat.hip: tophat_split_form, what launch_runs asks
before it launches k_morph_split), through lt_tophat_split_form: geometry in, form out.  No GPU.

The form needs rows that are 4-byte aligned, at most four bands (the waves of one workgroup are the bands of a task), and every
band -- the last, shorter one included -- at least one boundary zone long: 2R rounded up to the walk's rows per trip, 56 rows
for 55x55 (four rows per trip) and 28 for 29x29 (two)."""
import pytest


@pytest.fixture(scope="module")
def form():
    from lane_tracker_amd import _native
    lib = _native.load()
    return lambda h, w, k, nb: lib.lt_tophat_split_form(h, w, k, nb)


def test_production_geometry_splits(form):
    assert form(1100, 1080, 55, 4) == 1 and form(1100, 1080, 29, 4) == 1     # 4 bands of 275 rows
    assert form(1100, 1080, 55, 3) == 1 and form(1100, 1080, 55, 2) == 1 and form(1100, 1080, 29, 1) == 1


def test_band_count_against_the_workgroup_limit(form):
    for k in (29, 55):
        assert form(1100, 1080, k, 4) == 1
        assert form(1100, 1080, k, 5) == 0 and form(1100, 1080, k, 8) == 0   # 220-row bands would be long enough: the limit is the workgroup
        assert form(1100, 1080, k, 0) == 0


def test_zone_length_against_the_last_band(form):
    # 4 bands of ceil(h / 4) rows; last = h - 3 * ceil(h / 4)
    assert form(236, 188, 55, 4) == 1          # 59, 59, 59, 59
    assert form(233, 188, 55, 4) == 1          # 59, 59, 59, 56: exactly one 55x55 zone
    assert form(226, 188, 55, 4) == 0          # 57, 57, 57, 55: one row short
    assert form(226, 188, 29, 4) == 1          # ... and two 29x29 zones long
    assert form(224, 188, 55, 4) == 1          # 56 x 4
    assert form(223, 188, 55, 4) == 0          # 56, 56, 56, 55
    assert form(220, 188, 55, 4) == 0          # 55-row bands
    assert form(112, 188, 29, 4) == 1 and form(111, 188, 29, 4) == 0 and form(108, 188, 29, 4) == 0
    assert form(85, 188, 29, 4) == 0           # 22-row bands: ceil(85 / 22) = 4 bands, all shorter than a zone
    # a band count the height does not give (ceil(h / ceil(h / nb)) != nb) is still judged on the bands it does give
    assert form(57, 188, 29, 4) == 0


def test_alignment_and_structuring_elements(form):
    assert form(1100, 1082, 55, 4) == 0 and form(1100, 1081, 29, 4) == 0     # rows not 4-byte aligned: the byte-store kernels
    assert form(1100, 2, 29, 4) == 0
    assert form(1100, 1080, 5, 4) == 0 and form(1100, 1080, 31, 4) == 0      # only the 29x29 and 55x55 walks exist
    assert form(0, 1080, 55, 4) == 0 and form(1100, 0, 55, 4) == 0
