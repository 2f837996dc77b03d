"""tests/morph_reference.py -- the definition the top-hat form matrix compares the kernels with -- against two implementations
that share no code with it: scipy.ndimage's grey morphology on the ellipse's footprint (a tap outside the image is the neutral
value, mode="constant"), and the oracle.  A handful of planes, heights and widths below K included.  No GPU."""
import numpy as np
import pytest
from scipy import ndimage as ndi

import morph_reference as MR
from independent_tables import SURVEY_TAPS

SIZES = [(1, 1), (1, 70), (7, 3), (13, 61), (14, 15), (28, 29), (40, 131), (57, 64), (90, 33)]      # (h, w)


def _planes(h, w):
    rng = np.random.default_rng(1000 * h + w)
    y, x = np.mgrid[0:h, 0:w]
    sparse = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u = rng.random((h, w))
    sparse[u < 0.02] = 0
    sparse[u > 0.98] = 255
    deltas = np.full((h, w), 255, np.uint8)
    deltas[rng.integers(0, h, 3), rng.integers(0, w, 3)] = 0
    return {"noise": rng.integers(0, 256, (h, w), dtype=np.uint8), "sparse": sparse, "ramp": ((x + y) & 255).astype(np.uint8),
            "deltas": deltas, "inverse deltas": 255 - deltas}


@pytest.mark.parametrize("k", [29, 55])
def test_footprint_is_the_ellipse(k):
    from oracle import oracle as O
    fp = MR.footprint(k)
    assert fp.sum() == SURVEY_TAPS[k]
    assert np.array_equal(fp, O.ellipse_kernel(k) != 0)
    assert np.array_equal(fp, fp[::-1]) and np.array_equal(fp, fp[:, ::-1])


@pytest.mark.parametrize("k", [29, 55])
@pytest.mark.parametrize("size", SIZES)
def test_definition_equals_scipy_and_the_oracle(size, k):
    from oracle import oracle as O
    h, w = size
    fp = MR.footprint(k)
    for name, a in _planes(h, w).items():
        er, di, th = MR.erode(a, k), MR.dilate(a, k), MR.tophat(a, k)
        assert er.dtype == di.dtype == th.dtype == np.uint8
        assert np.array_equal(er, ndi.grey_erosion(a, footprint=fp, mode="constant", cval=255)), (name, "erode / scipy")
        assert np.array_equal(di, ndi.grey_dilation(a, footprint=fp, mode="constant", cval=0)), (name, "dilate / scipy")
        assert np.array_equal(er, O.erode(a, k)), (name, "erode / oracle")
        assert np.array_equal(di, O.dilate(a, k)), (name, "dilate / oracle")
        assert np.array_equal(th, O.tophat(a, k)), (name, "top-hat / oracle")
        opened = ndi.grey_dilation(ndi.grey_erosion(a, footprint=fp, mode="constant", cval=255), footprint=fp, mode="constant", cval=0)
        assert np.array_equal(th, a - opened), (name, "top-hat / scipy")
