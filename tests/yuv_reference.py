"""The YUV 4:2:0 -> RGB conversion restated in NumPy (int64), independently of the library: OpenCV's 20-bit fixed-point
arithmetic, one (U, V) pair per 2 x 2 block, no chroma interpolation.  `rgb_to_yuv420` only makes inputs.  Test infrastructure."""
import numpy as np

MATRICES = {"bt601": (1220542, 1673527, -852492, -409993, 2116026),     # CY, CVR, CVG, CUG, CUB (video range; OpenCV's)
            "bt709": (1220542, 1880097, -558891, -223347, 2214593)}


def convert_triples(y, u, v, matrix="bt601"):
    """(Y, U, V) integer arrays of one shape -> (..., 3) uint8 RGB."""
    cy, cvr, cvg, cug, cub = MATRICES[matrix] if isinstance(matrix, str) else matrix
    y, u, v = (np.asarray(a, np.int64) for a in (y, u, v))
    yy = np.maximum(0, y - 16) * cy + (1 << 19)
    r = (yy + cvr * (v - 128)) >> 20
    g = (yy + cvg * (v - 128) + cug * (u - 128)) >> 20
    b = (yy + cub * (u - 128)) >> 20
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def split_planes(frame, layout):
    """(H * 3 // 2, W) -> Y (H, W), U and V (H // 2, W // 2)."""
    frame = np.asarray(frame)
    h, w = frame.shape[0] * 2 // 3, frame.shape[1]
    assert frame.shape[0] * 2 == h * 3 and h % 2 == 0 and w % 2 == 0, frame.shape
    c = frame[h:].reshape(-1)
    if layout == "nv12":
        uv = c.reshape(h // 2, w // 2, 2)
        return frame[:h], uv[..., 0], uv[..., 1]
    assert layout == "i420", layout
    q = (h // 2) * (w // 2)
    return frame[:h], c[:q].reshape(h // 2, w // 2), c[q:].reshape(h // 2, w // 2)


def yuv420_to_rgb(frame, layout="nv12", matrix="bt601"):
    y, u, v = split_planes(frame, layout)
    up = lambda p: np.repeat(np.repeat(p, 2, 0), 2, 1)
    return convert_triples(y, up(u), up(v), matrix)


def rgb_to_yuv420(rgb, layout="nv12"):
    """An RGB image (H, W, 3), H and W even -> a 4:2:0 frame (BT.601 video range, float, rounded; chroma = mean of each 2 x 2 block)."""
    f = np.asarray(rgb, np.float64)
    h, w = f.shape[:2]
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 0.257 * r + 0.504 * g + 0.098 * b + 16
    u = -0.148 * r - 0.291 * g + 0.439 * b + 128
    v = 0.439 * r - 0.368 * g - 0.071 * b + 128
    mean = lambda p: p.reshape(h // 2, 2, w // 2, 2).mean((1, 3))
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    y, u, v = q(y), q(mean(u)), q(mean(v))
    chroma = np.stack([u, v], -1).reshape(-1) if layout == "nv12" else np.concatenate([u.reshape(-1), v.reshape(-1)])
    return np.concatenate([y.reshape(-1), chroma]).reshape(h * 3 // 2, w)
