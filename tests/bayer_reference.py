"""The 8-bit raw Bayer input restated in NumPy: the bilinear demosaic that `include/lane_tracker_amd.h` defines, vectorised, in two
forms that must agree -- the border form (interior pixels, then column 0 := column 1, column W - 1 := column W - 2, then rows 0 and
H - 1 from rows 1 and H - 2) and the clamp form (the demosaic at (clamp(y, 1, H - 2), clamp(x, 1, W - 2)) with that position's own
colour phase), which is the one the kernels use.  This is what `cv2.cvtColor(frame, cv2.COLOR_BayerRGGB2RGB)` (GRBG / GBRG / BGGR)
is understood to compute; that claim is checked only where OpenCV imports (test_bayer_cpu.py), the definition is the contract.

Test infrastructure: never imported by the product."""
import numpy as np

PATTERNS = ("bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr")
LAYOUT = {"bayer_rggb": 16, "bayer_grbg": 17, "bayer_gbrg": 18, "bayer_bggr": 19}
CHANNEL = {"r": 0, "g": 1, "b": 2}


def colour_at(pattern, y, x):
    """The channel (0 R, 1 G, 2 B) the mosaic carries at (y, x): position 2 * (y & 1) + (x & 1) of the pattern's name."""
    return CHANNEL[pattern[len("bayer_"):][2 * (y & 1) + (x & 1)]]


def colour_map(pattern, h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    tile = np.array([[colour_at(pattern, 0, 0), colour_at(pattern, 0, 1)], [colour_at(pattern, 1, 0), colour_at(pattern, 1, 1)]])
    return tile[ys & 1, xs & 1]


def check_mosaic(m):
    m = np.asarray(m)
    if m.dtype != np.uint8 or m.ndim != 2 or m.shape[0] % 2 or m.shape[1] % 2 or m.shape[0] < 4 or m.shape[1] < 4:
        raise ValueError("a raw Bayer frame is a uint8 array (H, W), H and W even and at least 4, got %s %r" % (m.dtype, m.shape))
    return m.astype(np.int32)


def _demosaic_at(m, pattern, ys, xs):
    """RGB at the interior positions (ys, xs) (index arrays of one shape, 1 <= y <= H - 2, 1 <= x <= W - 2) of the int32 mosaic m."""
    c = m[ys, xs]
    hs = m[ys, xs - 1] + m[ys, xs + 1]
    vs = m[ys - 1, xs] + m[ys + 1, xs]
    ds = m[ys - 1, xs - 1] + m[ys - 1, xs + 1] + m[ys + 1, xs - 1] + m[ys + 1, xs + 1]
    own = colour_map(pattern, *m.shape)[ys, xs]                  # the site's own colour
    horiz = colour_map(pattern, *m.shape)[ys, xs - 1]            # ... and that of its horizontal neighbours (a green site's: red or blue)
    out = np.zeros(c.shape + (3,), np.int32)
    green = own == 1
    for ch in (0, 2):                                            # red, blue
        at_own = own == ch                                       # a site of this colour: its own sample
        at_other = ~green & ~at_own                              # a site of the opposite colour: the four diagonal neighbours
        g_h = green & (horiz == ch)                              # a green site with this colour left and right
        g_v = green & (horiz != ch)                              # ... above and below
        out[..., ch] = np.where(at_own, c, np.where(at_other, (ds + 2) >> 2, np.where(g_h, (hs + 1) >> 1, (vs + 1) >> 1)))
        assert (at_own.astype(int) + at_other + g_h + g_v == 1).all()
    out[..., 1] = np.where(green, c, (hs + vs + 2) >> 2)
    return out.astype(np.uint8)


def bayer_to_rgb(mosaic, pattern):
    """The clamp form: (H, W) -> (H, W, 3); a stack (n, H, W) -> (n, H, W, 3)."""
    a = np.asarray(mosaic)
    if a.ndim == 3:
        return np.stack([bayer_to_rgb(f, pattern) for f in a]) if len(a) else np.zeros(a.shape + (3,), np.uint8)
    m = check_mosaic(a)
    h, w = m.shape
    ys, xs = np.mgrid[0:h, 0:w]
    return _demosaic_at(m, pattern, np.clip(ys, 1, h - 2), np.clip(xs, 1, w - 2))


def bayer_to_rgb_border(mosaic, pattern):
    """The border form: interior pixels demosaiced, then the border columns from their neighbours, then the border rows, whole."""
    m = check_mosaic(mosaic)
    h, w = m.shape
    out = np.zeros((h, w, 3), np.uint8)
    ys, xs = np.mgrid[1:h - 1, 1:w - 1]
    out[1:h - 1, 1:w - 1] = _demosaic_at(m, pattern, ys, xs)
    out[:, 0] = out[:, 1]
    out[:, w - 1] = out[:, w - 2]
    out[0] = out[1]
    out[h - 1] = out[h - 2]
    return out


def rgb_to_bayer(rgb, pattern):
    """The mosaic of an RGB picture (..., H, W, 3): every site keeps the channel the pattern gives it."""
    a = np.asarray(rgb)
    h, w = a.shape[-3], a.shape[-2]
    cm = colour_map(pattern, h, w)
    return np.ascontiguousarray(np.take_along_axis(a, np.broadcast_to(cm[..., None], a.shape[:-1] + (1,)), axis=-1)[..., 0])
