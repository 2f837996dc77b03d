"""The definition the top-hat kernels are held to (tests/test_gpu_tophat_forms.py): erode, dilate and top-hat with OpenCV's
k x k ellipse, in NumPy integers.

The footprint is one horizontal run per row, half-width dx[i] for footprint row i (independent_tables.ellipse_halfwidths_exact: the
ellipse in exact integer arithmetic).  A tap outside the image is ignored, as morphologyEx does with its default border.  The loop
below goes over the K footprint rows and takes a shifted minimum / maximum of the whole plane for each of the row's 2 dx + 1 taps (641
and 2337 shifts): no nested windows, no chain of doubled half-widths, no bands, no strips -- nothing of the kernels' run decomposition
(csrc/k_tophat.hip).
tests/test_morph_reference_cpu.py holds it equal to scipy.ndimage's grey morphology on the footprint and to the oracle."""
import numpy as np

from independent_tables import ellipse_halfwidths_exact


def footprint(k):
    """The k x k ellipse as a boolean array."""
    dx, _ = ellipse_halfwidths_exact(k)
    r = k // 2
    fp = np.zeros((k, k), bool)
    for i, d in enumerate(dx):
        fp[i, r - d:r + d + 1] = True
    return fp


def _morph(img, k, dilate):
    a = np.asarray(img)
    assert a.ndim == 2 and a.dtype == np.uint8
    h, w = a.shape
    r = k // 2
    dx, _ = ellipse_halfwidths_exact(k)
    neutral = 0 if dilate else 255
    op = np.maximum if dilate else np.minimum
    # the image in a frame of neutral values r wide: a tap outside the image never decides a minimum / maximum
    big = np.full((h + 2 * r, w + 2 * r), neutral, np.uint8)
    big[r:r + h, r:r + w] = a
    out = np.full((h, w), neutral, np.uint8)
    for i, d in enumerate(dx):                 # footprint row i reads image row y + i - r ...
        rows = big[i:i + h]
        for t in range(-d, d + 1):             # ... at columns x + t: the whole plane shifted by one tap
            op(out, rows[:, r + t:r + t + w], out=out)
    return out


def erode(img, k):
    return _morph(img, k, False)


def dilate(img, k):
    return _morph(img, k, True)


def tophat(img, k):
    """src - dilate(erode(src)); an opening never exceeds its source, so the difference needs no saturation -- asserted."""
    a = np.asarray(img)
    opened = dilate(erode(a, k), k)
    assert (opened <= a).all()
    return (a.astype(np.int32) - opened).astype(np.uint8)
