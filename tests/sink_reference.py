"""The RGB -> YUV 4:2:0 conversion of the device sinks restated in NumPy (int64), independently of the library: OpenCV's 20-bit
fixed-point arithmetic (cv2.cvtColor(img, COLOR_RGB2YUV_I420)), chroma from the pixel at the even row and even column of each
2 x 2 block, no averaging.  Test infrastructure."""
import numpy as np

# CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV (video range)
MATRICES = {"bt601": (269484, 528482, 102760, -155188, -305135, 460324, -385875, -74448),      # OpenCV's
            "bt709": (191455, 644067, 65019, -105533, -355018, 460551, -418321, -42230)}
# an accepted matrix scaled so that the clamps act at both ends of Y, U and V: every row has sum |c| = 7.5e6, which keeps
# sum |c| * 255 + 2^19 + (128 << 20) = 2.05e9 inside int32; yellow gives Y = 1596 -> 255, blue Y < 0 -> 0, and so on
CLAMPING = (3000000, 3500000, -1000000, -3000000, -1000000, 3500000, -3000000, -1000000)

# the float matrices the integers stand for: BT.601 as OpenCV rounds it to three digits, BT.709 exactly (Kr = 0.2126, Kb = 0.0722)
_KR, _KB = 0.2126, 0.0722
_KG = 1.0 - _KR - _KB
FLOAT_MATRICES = {
    "bt601": (0.257, 0.504, 0.098, -0.148, -0.291, 0.439, -0.368, -0.071),
    "bt709": (_KR * 219 / 255, _KG * 219 / 255, _KB * 219 / 255,
              -_KR / (2 * (1 - _KB)) * 224 / 255, -_KG / (2 * (1 - _KB)) * 224 / 255, 0.5 * 224 / 255,
              -_KG / (2 * (1 - _KR)) * 224 / 255, -_KB / (2 * (1 - _KR)) * 224 / 255)}


def coeffs(matrix):
    return tuple(int(v) for v in (MATRICES[matrix] if isinstance(matrix, str) else matrix))


def forward_triples(r, g, b, matrix="bt601"):
    """(R, G, B) integer arrays of one shape -> (Y, U, V) uint8 arrays: the three formulas of the issue, clamp to 0..255."""
    cry, cgy, cby, cru, cgu, cbu, cgv, cbv = coeffs(matrix)
    r, g, b = (np.asarray(a, np.int64) for a in (r, g, b))
    half = 1 << 19
    y = (cry * r + cgy * g + cby * b + half + (16 << 20)) >> 20
    u = (cru * r + cgu * g + cbu * b + half + (128 << 20)) >> 20
    v = (cbu * r + cgv * g + cbv * b + half + (128 << 20)) >> 20
    return tuple(np.clip(p, 0, 255).astype(np.uint8) for p in (y, u, v))


def rgb_to_yuv420(rgb, layout="nv12", matrix="bt601"):
    """RGB (..., H, W, 3), H and W even -> 4:2:0 frames (..., H * 3 // 2, W): Y plane, then U,V pairs ('nv12') or U plane, V plane."""
    rgb = np.asarray(rgb)
    lead, (h, w) = rgb.shape[:-3], rgb.shape[-3:-1]
    assert h % 2 == 0 and w % 2 == 0 and rgb.shape[-1] == 3, rgb.shape
    y, _, _ = forward_triples(rgb[..., 0], rgb[..., 1], rgb[..., 2], matrix)
    tl = rgb[..., 0::2, 0::2, :]
    _, u, v = forward_triples(tl[..., 0], tl[..., 1], tl[..., 2], matrix)
    flat = lambda p: p.reshape(lead + (-1,))
    chroma = flat(np.stack([u, v], -1)) if layout == "nv12" else np.concatenate([flat(u), flat(v)], -1)
    assert layout in ("nv12", "i420"), layout
    return np.concatenate([flat(y), chroma], -1).reshape(lead + (h * 3 // 2, w))


def all_colours():
    """The 2^24 (R, G, B) triples as three flat int64 arrays."""
    v = np.arange(256, dtype=np.int64)
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    return r.reshape(-1), g.reshape(-1), b.reshape(-1)
