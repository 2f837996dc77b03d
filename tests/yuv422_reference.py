"""The packed YUV 4:2:2 -> RGB conversion restated in NumPy, independently of the library: the per-pixel arithmetic is
`yuv_reference.convert_triples` (OpenCV's 20-bit fixed point), with the (U, V) pair of a macropixel repeated over its two pixels and
no chroma interpolation -- cv2.cvtColor(frame, COLOR_YUV2RGB_YUY2 / _UYVY).  A frame is a u8 array (H, W, 2), W even, as OpenCV holds
it: a row is W / 2 macropixels of four bytes, 'yuy2': Y0 U Y1 V, 'uyvy': U Y0 V Y1.  `rgb_to_yuv422` only makes inputs.  Test
infrastructure."""
import numpy as np

import yuv_reference as R

# byte positions of (Y0, U, Y1, V) inside a macropixel
ORDERS = {"yuy2": (0, 1, 2, 3), "uyvy": (1, 0, 3, 2)}


def split_422(frame, layout):
    """(H, W, 2) -> Y (H, W), U and V (H, W // 2)."""
    frame = np.asarray(frame)
    assert frame.ndim == 3 and frame.shape[2] == 2 and frame.shape[1] % 2 == 0, frame.shape
    h, w = frame.shape[:2]
    m = frame.reshape(h, w // 2, 4)
    y0, u, y1, v = (m[..., i] for i in ORDERS[layout])
    return np.stack([y0, y1], -1).reshape(h, w), u, v


def yuv422_to_rgb(frame, layout="yuy2", matrix="bt601"):
    y, u, v = split_422(frame, layout)
    return R.convert_triples(y, np.repeat(u, 2, 1), np.repeat(v, 2, 1), matrix)


def pack_422(y, u, v, layout):
    """Y (H, W), U and V (H, W // 2) -> the frame (H, W, 2)."""
    h, w = y.shape
    m = np.empty((h, w // 2, 4), np.uint8)
    for src, i in zip((y[:, 0::2], u, y[:, 1::2], v), ORDERS[layout]):
        m[..., i] = src
    return m.reshape(h, w, 2)


def rgb_to_yuv422(rgb, layout="yuy2"):
    """An RGB image (H, W, 3), W even -> a 4:2:2 frame (BT.601 video range, float, rounded; chroma = mean of each pixel pair)."""
    f = np.asarray(rgb, np.float64)
    h, w = f.shape[:2]
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 0.257 * r + 0.504 * g + 0.098 * b + 16
    u = -0.148 * r - 0.291 * g + 0.439 * b + 128
    v = 0.439 * r - 0.368 * g - 0.071 * b + 128
    mean = lambda p: p.reshape(h, w // 2, 2).mean(2)
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    return pack_422(q(y), q(mean(u)), q(mean(v)), layout)
