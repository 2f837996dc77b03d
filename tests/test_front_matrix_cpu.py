"""The inputs of the front end's matrix (front_matrix.py) must be able to catch what they are for: calibration sets that differ
on most pixels of the test's own frames, taps outside the image, an id pattern that puts every set on both slots of a pair and
changes across the chunk boundary, and a reference that is the composition the per-format suites already use.  No GPU."""
import itertools

import numpy as np
import pytest

import bayer_reference as RB
import front_matrix as FM
import yuv422_reference as R422
import yuv_reference as R420

CASES = FM.cases()
IDS = ["%s-%s" % c for c in CASES]


def test_the_sizes_are_the_ones_that_take_the_other_kernels():
    (wa, ha), (wb, hb), (wc, hc) = (FM.SIZES[s] for s in "ABC")
    assert wa % 4 == 0 and (wa * ha * 3) % 4 == 0                       # k_warp_split4 / k_warp_cal<4>, aligned RGB
    assert wb % 4 and (wb * 3) % 4 and wb * 3 == 198                    # k_warp_split1 / k_warp_cal<1>, 24-bit rows off the dword
    assert wb % 2 == 0 and hb % 2 == 0 and wa % 2 == 0 and ha % 2 == 0  # the YUV formats exist at A and B
    assert wc % 2 and hc % 2 and wc * hc * 3 == 2331 and 2331 % 4       # frames 2331 bytes apart: the unaligned RGB forms
    assert FM.formats_of("C") == FM.RGB_FAMILY and set(FM.formats_of("A")) == set(FM.formats_of("B")) == set(FM.FORMATS)
    assert FM.yuv_matrix("A") == "bt601" and FM.yuv_matrix("B") == "bt709"


@pytest.mark.parametrize("fmt,size", CASES, ids=IDS)
def test_every_two_sets_differ_on_three_quarters_of_the_pixels(fmt, size, oracle):
    """A condition on the inputs, not a tolerance: a wrong table or a wrong id cannot hide behind similar sets.  Measured at the
    worst: 0.91 of the undistorted pixels, 0.91 of the R plane (the YUV formats, whose R saturates), 0.98 of the Lab-b plane."""
    for k in (0, 1, FM.CAPACITY - 1):
        refs = [FM.reference(fmt, size, s, k) for s in range(FM.N_SETS)]
        for a, b in itertools.combinations(range(FM.N_SETS), 2):
            for what, x, y in zip(("undistorted", "R", "Lab-b"), refs[a], refs[b]):
                diff = (x != y).any(-1) if x.ndim == 3 else x != y
                print(fmt, size, "frame", k, "sets", a, b, what, round(float(diff.mean()), 3))
                assert diff.mean() >= 0.75, (fmt, size, k, a, b, what, float(diff.mean()))
    # ... and every two frames of the pool differ: a slot that shows its neighbour's frame shows it
    pool = FM.rgb_pool(fmt, size)
    assert len({p.tobytes() for p in pool}) == FM.CAPACITY


@pytest.mark.parametrize("size", list(FM.SIZES))
def test_border_taps_fractions_and_rows(size, oracle):
    w, h = FM.SIZES[size]
    stats = [FM.tap_stats(size, s) for s in range(FM.N_SETS)]
    rows = [FM.source_rows(size, s) for s in range(FM.N_SETS)]
    print(size, stats, rows)
    partly, fully, _ = stats[1]
    assert partly >= 0.03 and fully >= 0.10, stats[1]
    for s in (1, 2, 3):
        assert stats[s][2] >= 0.90, (s, stats[s])
    for s, (r0, r1) in enumerate(rows):
        assert 0 <= r0 and r1 <= h and r1 - r0 >= 5, (s, r0, r1)
    union = (min(r[0] for r in rows), max(r[1] for r in rows))
    assert union == (0, h) == rows[0]                                   # the identity reads every row: the context's rows are the image
    assert union[0] < rows[2][0] and rows[2][1] < union[1], rows        # set 2: a narrow run, strictly inside
    # the second remap has taps outside as well: some bird's-eye pixel of set 1 lies outside the camera image
    xy, _ = oracle.warp_map(FM.oracle_calib(size, 1))
    sx, sy = xy[..., 0].astype(int), xy[..., 1].astype(int)
    assert ((sx < 0) | (sx + 1 >= w) | (sy < 0) | (sy + 1 >= h)).any()


def test_the_id_pattern_reaches_every_set_on_both_slots_of_a_pair_and_changes_at_the_chunk():
    ids = FM.ids_pattern(67)
    assert len(ids) == 67 and set(ids) == set(range(FM.N_SETS))
    for first in FM.FIRSTS:
        for parity in (0, 1):
            assert {s for i, s in enumerate(ids) if (first + i) % 2 == parity} == set(range(FM.N_SETS)), (first, parity)
    assert ids[63] != ids[64]                                           # across the boundary of a chunk of 64 ...
    assert len(set(ids[64:])) >= 2                                      # ... and a second chunk that is mixed itself
    assert ids[:5] == FM.ids_pattern(5) and len(set(ids[:5])) == FM.N_SETS       # the short range: one chunk, all four sets
    assert ids[64:] != ids[:3]                                          # ids + i, not ids, or the second chunk shows it
    tail = FM.ids_pattern(FM.CAPACITY // 2)                             # the second slice of the two-stream row
    assert len(set(tail)) == FM.N_SETS


def test_alternating_runs_cover_the_range_in_runs_of_one_two_three():
    for n in (1, 3, 5, 37, 67, 72):
        runs = FM.alternating_runs(n)
        assert runs[0][0] == 0 and runs[-1][1] == n and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
        assert [b - a for a, b, _ in runs[:-1]] == [1 + k % 3 for k in range(len(runs) - 1)]
        assert all(x[2] != y[2] for x, y in zip(runs, runs[1:])) and runs[0][2]
    runs = FM.alternating_runs(67)
    assert any(a < 64 < b for a, b, _ in runs)                          # a run that the chunk boundary cuts
    assert {att for a, b, att in runs if b > 64} == {True, False}       # both kinds behind it


@pytest.mark.parametrize("fmt", FM.FORMATS)
def test_the_reference_is_the_composition_the_format_suites_use(fmt, oracle):
    """to_rgb() of the format's own definition, then the oracle: on one frame per format and size."""
    from lane_tracker_amd import utils
    for size in ("A", "B", "C"):
        if fmt not in FM.formats_of(size):
            continue
        k, s = 5, 3
        frame = FM.frame_pool(fmt, size)[k]
        assert frame.shape == FM.frame_shape(fmt, size) and frame.dtype == np.uint8
        m = FM.yuv_matrix(size)
        if fmt in R422.ORDERS:
            rgb = R422.yuv422_to_rgb(frame, fmt, m)
        elif fmt in ("nv12", "i420"):
            rgb = R420.yuv420_to_rgb(frame, fmt, m)
        elif fmt in RB.PATTERNS:
            rgb = RB.bayer_to_rgb(frame, fmt)
            assert np.array_equal(rgb, RB.bayer_to_rgb_border(frame, fmt))
        elif fmt == "rgb":
            rgb = frame
        else:                                                           # the permutation that packs RGB into the format, undone
            rgb = FM.to_rgb(frame, fmt)
            packed = utils.rgb_to_packed(rgb, fmt)
            assert np.array_equal(packed[..., :3], frame[..., :3])
            assert np.array_equal(rgb, {"bgr": frame[..., ::-1], "rgba": frame[..., :3], "bgra": frame[..., 2::-1]}[fmt])
        assert np.array_equal(FM.rgb_pool(fmt, size)[k], rgb)
        oc = FM.oracle_calib(size, s)
        und, r, b = FM.reference(fmt, size, s, k)
        assert np.array_equal(und, oracle.undistort(oc, rgb))
        bev = oracle.warp(oc, und)                                      # the two remaps one after the other are the front end
        assert np.array_equal(bev, oracle.front_end(oc, rgb))
        assert np.array_equal(r, bev[..., 0]) and np.array_equal(b, oracle.lab_b(bev))
        assert und.shape == FM.SIZES[size][::-1] + (3,) and r.shape == b.shape == FM.SIZES[size][::-1]


@pytest.mark.parametrize("fmt,size", CASES, ids=IDS)
def test_surfaces_are_pitched_offset_and_end_on_their_last_byte(fmt, size):
    frames = FM.frame_pool(fmt, size)[:3]
    w, h = FM.SIZES[size]
    pitch, cp = FM.surface_pitches(fmt, size)
    for offset in range(4):
        block, surf = FM.pack_surfaces(frames, fmt, size, offset)
        assert int(surf["plane"][0, 0]) == offset and (block[:offset] == FM.FILL).all()
        assert (surf["pitch"] == pitch).all() and (surf["chroma_pitch"] == (cp or 0)).all()
        flat = frames.reshape(3, -1)
        row_bytes = flat.shape[1] // h if cp is None else w
        assert pitch == row_bytes + 5
        last = {"nv12": (1, h // 2, w, cp), "i420": (2, h // 2, w // 2, cp)}.get(fmt, (0, h, row_bytes, pitch))
        plane, rows, rb, p = last
        end = int(surf["plane"][2, plane]) + p * (rows - 1) + rb
        assert end == block.size                                        # the last byte of the last row is the block's last
        assert np.array_equal(block[end - rb:], flat[2, -rb:])
        first = np.lib.stride_tricks.as_strided(block[offset:], shape=(h, pitch), strides=(pitch, 1))
        assert np.array_equal(first[:, :row_bytes].reshape(-1), flat[0, :h * row_bytes])
        assert (first[:-1, row_bytes:] == FM.FILL).all()                # between the rows
