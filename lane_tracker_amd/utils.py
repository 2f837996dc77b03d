"""Calibration loaders with the reference's names and return values (reference utils.py:13-55).
Pickle files written by the reference (`cam_calib.p`, `warp_params.p`) load as before; `.npz` files
with the same keys load without unpickling anything."""
import collections
import pickle

import numpy as np


def _load_mapping(filepath):
    if str(filepath).endswith(".npz"):
        with np.load(filepath, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    with open(filepath, "rb") as f:
        return pickle.load(f)


def load_camera_calib(filepath):
    """-> (cam_matrix, dist_coeffs)"""
    d = _load_mapping(filepath)
    cam_matrix, dist_coeffs = d['cam_matrix'], d['dist_coeffs']
    print("Camera matrix and distortion coefficients loaded.")
    return cam_matrix, dist_coeffs


def load_warp_params(filepath):
    """-> (M, Minv, image_width_height, warped_width_height, mppv, mpph)"""
    d = _load_mapping(filepath)
    as_size = lambda v: tuple(int(t) for t in np.asarray(v).reshape(-1)[:2])
    out = (d['M'], d['Minv'], as_size(d['image_width_height']), as_size(d['warped_width_height']),
           float(d['mppv']), float(d['mpph']))
    print("Warp parameters loaded.")
    return out


def save_calibration_npz(cam_path, warp_path, cam_matrix, dist_coeffs, M, Minv, image_width_height,
                         warped_width_height, mppv, mpph):
    np.savez(cam_path, cam_matrix=np.asarray(cam_matrix), dist_coeffs=np.asarray(dist_coeffs))
    np.savez(warp_path, M=np.asarray(M), Minv=np.asarray(Minv), image_width_height=np.asarray(image_width_height),
             warped_width_height=np.asarray(warped_width_height), mppv=mppv, mpph=mpph)


def _resize_taps(src_len, dst_len):
    """cv2.resize INTER_LINEAR tap positions and 11-bit coefficients along one axis."""
    f = ((np.arange(dst_len, dtype=np.float64) + 0.5) * (src_len / dst_len) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    low, high = s < 0, s >= src_len - 1
    s = np.where(low, 0, np.where(high, src_len - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, src_len - 1), c0, c1


def resize_linear(img, dsize):
    """cv2.resize(img, dsize=(w, h)) with the default bilinear interpolation on u8 images: half-pixel
    centres, 11-bit coefficients, OpenCV's two-stage fixed-point rounding."""
    img = np.asarray(img, np.uint8)
    dw, dh = int(dsize[0]), int(dsize[1])
    x0, x1, a0, a1 = _resize_taps(img.shape[1], dw)
    y0, y1, b0, b1 = _resize_taps(img.shape[0], dh)
    src = img.astype(np.int64)
    if src.ndim == 3:
        a0, a1 = a0[None, :, None], a1[None, :, None]
        b0, b1 = b0[:, None, None], b1[:, None, None]
    else:
        a0, a1 = a0[None, :], a1[None, :]
        b0, b1 = b0[:, None], b1[:, None]
    rows = src[:, x0] * a0 + src[:, x1] * a1                     # horizontal pass, all source rows
    out = (((b0 * (rows[y0] >> 4)) >> 16) + ((b1 * (rows[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def create_split_view(target_size, images, positions, sizes, captions=[]):
    """Place images on a canvas of `target_size` (w, h) (reference utils.py:57-103): each image is
    resized to its slot with the bilinear `resize_linear`; one-channel images fill all three
    channels; captions are not rendered (they need OpenCV's Hershey glyphs)."""
    assert len(images) == len(positions) == len(sizes)
    x_max, y_max = target_size
    canvas = np.zeros((y_max, x_max, 3), dtype=np.uint8)
    for img, (x, y), (w, h) in zip(images, positions, sizes):
        if img.shape[0] != h or img.shape[1] != w:
            img = resize_linear(img, (w, h))
        if img.ndim == 2:
            img = img[:, :, None]
        canvas[y:min(y + h, y_max), x:min(x + w, x_max), :] = img[:min(h, y_max - y), :min(w, x_max - x)]
    return canvas


def yuv_to_rgb(frame, layout='nv12', matrix='bt601'):
    """A YUV 4:2:0 frame as OpenCV holds it -- a u8 array (H * 3 // 2, W): the Y plane, then interleaved U,V rows ('nv12') or the
    U plane and the V plane ('i420') -- to RGB (H, W, 3), on the device: `cv2.cvtColor(frame, cv2.COLOR_YUV2RGB_NV12)` /
    `_I420` bit for bit with matrix='bt601' (OpenCV's constants, video range); 'bt709' or five integers {CY, CVR, CVG, CUG, CUB}
    (20-bit fixed point) for another matrix.  Or a packed 4:2:2 frame as OpenCV holds it -- a u8 array (H, W, 2), W even: 'yuy2'
    (bytes Y0 U Y1 V) / 'uyvy' (U Y0 V Y1) -- `cv2.cvtColor(frame, cv2.COLOR_YUV2RGB_YUY2)` / `_UYVY`, the same arithmetic with one
    (U, V) pair per horizontal pixel pair.  What a `LaneTracker(..., pixel_format=layout, yuv_matrix=matrix)` sees of the frame."""
    from . import _native
    from .lane_tracker import _context_for_module_functions
    if not _native.is_yuv(_native.pixel_format_id(layout)):          # (before a context is made: 'rgb', 'bgr', 'rgba', 'bgra' hold no YUV)
        raise ValueError("layout must be 'nv12', 'i420', 'yuy2' or 'uyvy'")
    return _context_for_module_functions().yuv_to_rgb(frame, layout, matrix)


def bayer_to_rgb(frame, pattern='bayer_rggb', raw_lut=None):
    """An 8-bit raw Bayer frame -- a u8 array (H, W), H and W even and at least 4, the sensor's mosaic with `pattern` ('bayer_rggb',
    'bayer_grbg', 'bayer_gbrg', 'bayer_bggr': its top-left 2 x 2 block) -- or a stack (n, H, W) of them, to RGB (H, W, 3) /
    (n, H, W, 3), on the device: the bilinear demosaic in integers, border pixels taking their interior neighbours' values.  This is
    what `cv2.cvtColor(frame, cv2.COLOR_BayerRGGB2RGB)` (GRBG / GBRG / BGGR) is understood to compute, which was not checked against
    OpenCV.  What a `LaneTracker(..., pixel_format=pattern)` sees of the frame.

    The 10- and 12-bit patterns ('bayer10_rggb', ..., 'bayer12_bggr') take uint16 frames -- the sample in the low 10 / 12 bits of each
    word, the bits above ignored -- and look every sample up in `raw_lut`, u8 (4, 2**bits), first (None: the default
    `raw_lut(bits=...)`): the demosaic of `apply_raw_lut(frame, pattern, raw_lut)`.  `raw_lut` goes with these patterns only.

    The MIPI-packed patterns ('bayer10p_rggb', ..., 'bayer12p_bggr') take u8 frames of packed rows, (H, W * 5 // 4) / (H, W * 3 // 2)
    (`pack_raw`), and are otherwise the 10- / 12-bit patterns: unpacked on the device, on the way into the table."""
    from . import _native
    from .lane_tracker import _context_for_module_functions
    wide = pattern in _native.BAYER_DEEP_FORMATS
    if pattern not in _native.RAW_FORMATS:
        raise ValueError("pattern must be one of %s, got %r" % (", ".join(repr(n) for n in _native.RAW_FORMATS), pattern))
    if raw_lut is not None and not wide:
        raise ValueError("bayer_to_rgb takes a raw_lut with the 10- and 12-bit patterns only (8-bit: apply_raw_lut first)")
    raw_lut = _native.checked_raw_lut(raw_lut, pattern)
    a = _native.frames_array(frame, pattern)
    if a.ndim in (2, 3):                                 # (a size no raw frame has: refused before a context is made)
        _native.raw_frame_size(np.empty(a.shape[-2:], a.dtype), pattern)
    convert = (lambda ctx, f: ctx.bayer_to_rgb(f, pattern, raw_lut)) if wide else (lambda ctx, f: ctx.bayer_to_rgb(f, pattern))
    if a.ndim == 2:
        return convert(_context_for_module_functions(), a)
    if a.ndim != 3:
        raise ValueError("a raw Bayer frame is an array (H, W), a stack of them (n, H, W); got %r" % (a.shape,))
    ctx = _context_for_module_functions()
    if a.shape[0] == 0:
        return np.empty((0,) + _native.raw_frame_size(np.empty(a.shape[1:], a.dtype), pattern) + (3,), np.uint8)
    return np.stack([convert(ctx, a[k]) for k in range(a.shape[0])])


_BAYER_PATTERNS = ('bayer_rggb', 'bayer_grbg', 'bayer_gbrg', 'bayer_bggr')     # pattern p: its red sites at (row, column) parity (p >> 1, p & 1)
# the 10- and 12-bit forms: name -> (pattern p, bits)
_BAYER_WIDE_PATTERNS = {'bayer%d_%s' % (b, n[6:]): (p, b) for b in (10, 12) for p, n in enumerate(_BAYER_PATTERNS)}


# the same MIPI-packed: name -> (pattern p, bits)
_BAYER_PACKED_PATTERNS = {'bayer%dp_%s' % (b, n[6:]): (p, b) for b in (10, 12) for p, n in enumerate(_BAYER_PATTERNS)}


def _packed_bits(fmt):
    """The sample bits of a packed raw layout given as a name ('bayer10p_rggb', or '10p' / '12p' alone) or as 10 / 12."""
    if fmt in _BAYER_PACKED_PATTERNS:
        return _BAYER_PACKED_PATTERNS[fmt][1]
    if fmt in (10, 12, '10p', '12p'):
        return int(str(fmt)[:2])
    raise ValueError("fmt must be one of %s (or '10p' / '12p'), got %r" % (", ".join(repr(n) for n in _BAYER_PACKED_PATTERNS), fmt))


def pack_raw(frames, fmt):
    """10- / 12-bit raw Bayer frames in words -- uint16 (H, W) or a stack (n, H, W), every sample below 2**bits -- as MIPI packs them
    (CSI-2 RAW10 / RAW12; V4L2 SRGGB10P / SRGGB12P and siblings): u8 (..., H, W * 5 // 4) or (..., H, W * 3 // 2).

        RAW10 (W % 4 == 0): group g holds sites 4g .. 4g + 3; byte 5g + i is s[4g + i] >> 2 (i = 0 .. 3), bits 2i + 1 : 2i of byte
                            5g + 4 are s[4g + i] & 3
        RAW12 (W even):     byte 3g is s[2g] >> 4, byte 3g + 1 is s[2g + 1] >> 4, byte 3g + 2 is (s[2g] & 15) | (s[2g + 1] & 15) << 4

    `fmt`: a packed pixel format ('bayer10p_rggb', ...; the pattern plays no part) or '10p' / '12p'.  NumPy only."""
    bits = _packed_bits(fmt)
    a = np.asarray(frames)
    if a.dtype != np.uint16 or a.ndim not in (2, 3):
        raise ValueError("frames to pack are uint16 arrays (H, W) or (n, H, W), got %s %r" % (a.dtype, a.shape))
    per = 4 if bits == 10 else 2
    if a.shape[-1] % per or a.shape[-1] == 0:
        raise ValueError("RAW%d packs %d samples at a time: the width must be a multiple of %d, got %d" % (bits, per, per, a.shape[-1]))
    if a.size and int(a.max()) >> bits:
        raise ValueError("a %d-bit sample is below %d, got %d" % (bits, 1 << bits, int(a.max())))
    g = a.reshape(a.shape[:-1] + (a.shape[-1] // per, per))
    out = np.empty(g.shape[:-1] + (per + 1,), np.uint8)
    out[..., :per] = g >> (bits - 8)
    low = g & ((1 << (bits - 8)) - 1)
    out[..., per] = sum(low[..., i] << ((bits - 8) * i) for i in range(per))
    return out.reshape(a.shape[:-1] + (-1,))


def unpack_raw(frames, fmt):
    """The inverse of `pack_raw`, and the DEFINITION of the packed layouts: u8 packed rows (H, W * 5 // 4) / (H, W * 3 // 2), or a stack of
    them, -> uint16 (..., H, W).  A tracker or group in 'bayer10p_P' / 'bayer12p_P' fed packed frames F computes, bit for bit, what the one in
    'bayer10_P' / 'bayer12_P' with the same table, colour stage and shading map computes from `unpack_raw(F, fmt)`.  NumPy only."""
    bits = _packed_bits(fmt)
    a = np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError("packed frames are uint8 arrays (H, row bytes) or (n, H, row bytes), got %s %r" % (a.dtype, a.shape))
    per = 4 if bits == 10 else 2
    if a.shape[-1] % (per + 1) or a.shape[-1] == 0:
        raise ValueError("a RAW%d row is a multiple of %d bytes, got %d" % (bits, per + 1, a.shape[-1]))
    g = a.reshape(a.shape[:-1] + (a.shape[-1] // (per + 1), per + 1)).astype(np.uint16)
    out = np.empty(g.shape[:-1] + (per,), np.uint16)
    for i in range(per):
        out[..., i] = (g[..., i] << (bits - 8)) | ((g[..., per] >> ((bits - 8) * i)) & ((1 << (bits - 8)) - 1))
    return out.reshape(a.shape[:-1] + (-1,))


def pack_mask_bits(masks):
    """Binary masks (..., H, W), a pixel set where != 0 (u8 or bool), as the bit planes of `Context.upload_mask_bits`: uint64
    (..., H, (W + 63) // 64); pixel x of a row is bit x % 64 of the row's word x // 64, least significant bit first; the bits at
    columns >= W are zero.  NumPy only."""
    a = np.asarray(masks)
    if a.ndim < 2 or a.shape[-1] == 0:
        raise ValueError("masks to pack are arrays (..., H, W) with W > 0, got %r" % (a.shape,))
    w = a.shape[-1]
    wpr = (w + 63) // 64
    set_ = np.zeros(a.shape[:-1] + (wpr * 64,), np.uint8)
    set_[..., :w] = a != 0
    octets = set_.reshape(a.shape[:-1] + (wpr * 8, 8))
    by = np.zeros(octets.shape[:-1], np.uint8)
    for k in range(8):
        by |= octets[..., k] << k
    return np.ascontiguousarray(by).view('<u8').astype(np.uint64, copy=False).reshape(a.shape[:-1] + (wpr,))


def unpack_mask_bits(bits, width, value=255):
    """The inverse of `pack_mask_bits`: uint64 (..., H, wpr) -> u8 (..., H, width), `value` where the bit is set.  Bits at columns
    >= width are dropped.  NumPy only."""
    b = np.ascontiguousarray(np.asarray(bits, np.uint64).astype('<u8', copy=False))
    if b.ndim < 2 or not 0 < width <= 64 * b.shape[-1] or width <= 64 * (b.shape[-1] - 1):
        raise ValueError("a row of width %d is %d words, got %r" % (width, (width + 63) // 64, b.shape))
    by = b.view(np.uint8).reshape(b.shape[:-1] + (b.shape[-1] * 8, 1))
    set_ = (by >> np.arange(8, dtype=np.uint8)) & 1
    return (set_.reshape(b.shape[:-1] + (-1,))[..., :width] * np.uint8(value)).astype(np.uint8)


def checked_raw_lut(lut, bits=8):
    """A raw table as the C-contiguous u8 array (4, 256) -- (4, 2**bits) for 10- / 12-bit samples -- the device takes; ValueError for any
    other shape or dtype (nothing is cast: a float table is a mistake, not a table)."""
    a = np.asarray(lut)
    if a.dtype != np.uint8 or a.shape != (4, 1 << bits):
        raise ValueError("a raw table is a uint8 array of shape (4, %d), got %s %r" % (1 << bits, a.dtype, a.shape))
    return np.ascontiguousarray(a)


def raw_lut(black_level=0, white_level=None, gains=(1, 1, 1), gamma=1.0, bits=8):
    """The raw table -- u8 (4, 2**bits), bits = 8 (the default), 10 or 12: (4, 256) for 8-bit samples --, one row per colour phase: 0 red sites, 1 green on red rows, 2 green on blue rows, 3 blue sites --
    of the three steps every raw pipeline applies before demosaicing: black-level subtraction, per-colour gains (white balance) and
    a tone curve.  For a sample s = 0 .. 2**bits - 1 of the colour with gain g, in float64 (white_level: 2**bits - 1 unless given):

        v = clip((s - black_level) / (white_level - black_level), 0, 1)
        v = clip(v * g, 0, 1)
        v = v ** (1 / gamma)           gamma='srgb':  12.92 v  if v <= 0.0031308  else  1.055 v ** (1 / 2.4) - 0.055
        out = floor(255 v + 0.5)

    `gains` is (R, G, B) or (R, Gr, Gb, B); `gamma` a positive number or 'srgb'.  The defaults give the identity.  What
    `LaneTracker(..., pixel_format='bayer_*', raw_lut=...)` looks every sample up in; `apply_raw_lut` is the same on the host."""
    if bits not in (8, 10, 12):
        raise ValueError("bits is 8, 10 or 12, got %r" % (bits,))
    n = 1 << bits
    black, white = float(black_level), float(n - 1 if white_level is None else white_level)
    if not white > black:
        raise ValueError("white_level must be above black_level, got %r <= %r" % (n - 1 if white_level is None else white_level, black_level))
    g = [float(v) for v in gains]
    if len(g) == 3:
        g = [g[0], g[1], g[1], g[2]]
    if len(g) != 4:
        raise ValueError("gains are (R, G, B) or (R, Gr, Gb, B), got %d values" % len(g))
    if any(not v >= 0 for v in g):
        raise ValueError("gains must not be negative, got %r" % (tuple(gains),))
    if gamma != 'srgb' and (isinstance(gamma, str) or not float(gamma) > 0):
        raise ValueError("gamma is a positive number or 'srgb', got %r" % (gamma,))
    s = np.arange(n, dtype=np.float64)
    v = np.clip((s - black) / (white - black), 0.0, 1.0)
    out = np.empty((4, n), np.uint8)
    for p in range(4):
        t = np.clip(v * g[p], 0.0, 1.0)
        if gamma == 'srgb':
            t = np.where(t <= 0.0031308, 12.92 * t, 1.055 * t ** (1.0 / 2.4) - 0.055)
        else:
            t = t ** (1.0 / float(gamma))
        out[p] = np.floor(255.0 * t + 0.5).astype(np.uint8)
    return out


def apply_raw_lut(frames, pattern, lut):
    """The conditioned mosaic of 8-bit raw Bayer frames -- (H, W) or a stack (n, H, W) -- with `pattern` ('bayer_rggb', ...):
    out[y, x] = lut[phase(y, x)][frames[y, x]], phase = 2 * ((y ^ red_row) & 1) + ((x ^ red_col) & 1) with the pattern's red sites at
    (row, column) parity (red_row, red_col).  NumPy only.  This is the definition: a Bayer tracker with `raw_lut=lut` fed `frames`
    computes, bit for bit, what one without a table computes from `apply_raw_lut(frames, pattern, lut)`.

    The 10- and 12-bit patterns ('bayer10_rggb', ..., 'bayer12_bggr'): uint16 frames, a table u8 (4, 2**bits), and
    out[y, x] = lut[phase(y, x)][frames[y, x] & (2**bits - 1)], a uint8 mosaic -- the bits of a word above `bits` are ignored.  A tracker in
    'bayerNN_P' with table `lut` computes what the 8-bit 'bayer_P' tracker without a table computes from this.

    The MIPI-packed patterns ('bayer10p_*', 'bayer12p_*'): u8 packed rows, unpacked (`unpack_raw`) and then as the 10- / 12-bit patterns."""
    if pattern in _BAYER_PACKED_PATTERNS:
        return apply_raw_lut(unpack_raw(frames, pattern), pattern.replace("p_", "_", 1), lut)
    if pattern in _BAYER_WIDE_PATTERNS:
        p, bits = _BAYER_WIDE_PATTERNS[pattern]
        dtype = np.uint16
    elif pattern in _BAYER_PATTERNS:
        p, bits, dtype = _BAYER_PATTERNS.index(pattern), 8, np.uint8
    else:
        raise ValueError("pattern must be one of %s, got %r" % (", ".join(repr(n) for n in _BAYER_PATTERNS + tuple(_BAYER_WIDE_PATTERNS)), pattern))
    lut = checked_raw_lut(lut, bits)
    a = np.asarray(frames)
    if a.dtype != dtype or a.ndim not in (2, 3):
        raise ValueError("%s frames are %s arrays (H, W) or (n, H, W), got %s %r" % (pattern, np.dtype(dtype), a.dtype, a.shape))
    out = np.empty(a.shape, np.uint8)
    for py in range(2):
        for px in range(2):
            row = lut[2 * (py ^ (p >> 1)) + (px ^ (p & 1))]
            out[..., py::2, px::2] = row[a[..., py::2, px::2] & ((1 << bits) - 1)]
    return out


def checked_raw_ccm(ccm):
    """A colour-correction matrix as the C-contiguous int16 array (3, 3) the device takes; ValueError for any other shape or dtype
    (nothing is cast: a float matrix goes through `utils.raw_ccm` first)."""
    a = np.asarray(ccm)
    if a.dtype != np.int16 or a.shape != (3, 3):
        raise ValueError("a colour-correction matrix is an int16 array of shape (3, 3) in Q10 -- utils.raw_ccm makes one of a float "
                         "matrix --, got %s %r" % (a.dtype, a.shape))
    return np.ascontiguousarray(a)


def checked_raw_curve(curve):
    """An output curve as the C-contiguous u8 array (256,) the device takes; ValueError for any other shape or dtype."""
    a = np.asarray(curve)
    if a.dtype != np.uint8 or a.shape != (256,):
        raise ValueError("an output curve is a uint8 array of shape (256,), got %s %r" % (a.dtype, a.shape))
    return np.ascontiguousarray(a)


def raw_ccm(matrix, preserve_white=True):
    """A colour-correction matrix -- float 3 x 3, sensor RGB to display RGB, row c making output channel c -- as the int16 (3, 3) in Q10
    that the colour stage of a raw Bayer tracker takes (`LaneTracker(..., raw_ccm=...)`): rint(1024 m).  With `preserve_white` the
    diagonal entry of every row is then adjusted so that the row sums to rint(1024 * sum(row)): a matrix whose rows sum to 1 keeps grey
    grey, exactly.  ValueError for another shape, a value that is not finite, or an entry that leaves int16."""
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (3, 3):
        raise ValueError("a colour-correction matrix is 3 x 3, got %r" % (m.shape,))
    if not np.all(np.isfinite(m)):
        raise ValueError("a colour-correction matrix holds finite numbers, got %r" % (m.tolist(),))
    q = np.rint(1024.0 * m)
    if preserve_white:
        for c in range(3):
            q[c, c] += np.rint(1024.0 * m[c].sum()) - q[c].sum()
    if q.min() < -32768 or q.max() > 32767:
        raise ValueError("a colour-correction matrix in Q10 must fit int16 (entries -32 .. 31.999), got %r" % (m.tolist(),))
    return q.astype(np.int16)


def raw_curve(gamma=1.0):
    """An output curve, u8 (256,), for the colour stage of a raw Bayer tracker (`LaneTracker(..., raw_curve=...)`): the tone step of
    `raw_lut` on v = s / 255 --

        v = v ** (1 / gamma)           gamma='srgb':  12.92 v  if v <= 0.0031308  else  1.055 v ** (1 / 2.4) - 0.055
        out = floor(255 v + 0.5)

    -- for s = 0 .. 255.  gamma = 1 is the identity."""
    if gamma != 'srgb' and (isinstance(gamma, str) or not float(gamma) > 0):
        raise ValueError("gamma is a positive number or 'srgb', got %r" % (gamma,))
    t = np.arange(256, dtype=np.float64) / 255.0
    if gamma == 'srgb':
        t = np.where(t <= 0.0031308, 12.92 * t, 1.055 * t ** (1.0 / 2.4) - 0.055)
    else:
        t = t ** (1.0 / float(gamma))
    return np.floor(255.0 * t + 0.5).astype(np.uint8)


def apply_raw_color(rgb, ccm=None, curve=None):
    """The colour stage of raw Bayer input on u8 RGB (..., 3): with M = `ccm`, int16 (3, 3) in Q10 (None: 1024 * I), and T = `curve`,
    u8 (256,) (None: arange(256)),

        v[c]   = (M[c][0] * R + M[c][1] * G + M[c][2] * B + 512) >> 10        int32, arithmetic shift (floor)
        out[c] = T[min(max(v[c], 0), 255)]

    NumPy only.  This is the definition: a raw Bayer tracker with `raw_ccm=M, raw_curve=T` (and, if set, raw table L) fed frames F
    computes, bit for bit, what an RGB tracker computes from `apply_raw_color(bayer_to_rgb(apply_raw_lut(F, pattern, L), pattern), M, T)`."""
    m = np.eye(3, dtype=np.int32) * 1024 if ccm is None else checked_raw_ccm(ccm).astype(np.int32)
    t = np.arange(256, dtype=np.uint8) if curve is None else checked_raw_curve(curve)
    a = np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError("RGB pixels are a uint8 array (..., 3), got %s %r" % (a.dtype, a.shape))
    p = a.astype(np.int32)
    v = (p[..., None, :] * m).sum(axis=-1)                  # (..., 3): channel c from row c
    return t[np.clip((v + 512) >> 10, 0, 255)]


RawShading = collections.namedtuple("RawShading", "mesh black")
RawShading.__doc__ = """A lens-shading map of raw Bayer input: `mesh` uint16 (4, mh, mw), gains in Q12 (4096 is 1.0), one plane per colour
phase (0 red sites, 1 green on red rows, 2 green on blue rows, 3 blue sites), 2 <= mh, mw <= 64, node (0, 0) on pixel (0, 0) and node
(mh - 1, mw - 1) on the image's last pixel; `black` int32 (4,), the pedestal of each phase.  `utils.raw_shading` makes one."""
_MESH_MIN, _MESH_MAX = 2, 64


def _pattern_bits(pattern):
    """-> (pattern p, bits, dtype of the frames) of one of the twelve raw patterns."""
    if pattern in _BAYER_WIDE_PATTERNS:
        return _BAYER_WIDE_PATTERNS[pattern] + (np.uint16,)
    if pattern in _BAYER_PATTERNS:
        return _BAYER_PATTERNS.index(pattern), 8, np.uint8
    raise ValueError("pattern must be one of %s, got %r" % (", ".join(repr(n) for n in _BAYER_PATTERNS + tuple(_BAYER_WIDE_PATTERNS)), pattern))


def checked_raw_shading(shading, bits=8):
    """A shading map as RawShading(mesh C-contiguous uint16 (4, mh, mw), black int32 (4,)), as the device takes it; ValueError for
    anything that is not a (mesh, black) pair, another dtype or shape of the mesh (nothing is cast: float gains go through
    `utils.raw_shading` first), a mesh side outside 2 .. 64, or a black value outside 0 .. 2**bits - 1."""
    try:
        mesh, black = shading
    except (TypeError, ValueError):
        raise ValueError("a shading map is a utils.RawShading (mesh, black), got %r" % (type(shading).__name__,)) from None
    m = np.asarray(mesh)
    if m.dtype != np.uint16 or m.ndim != 3 or m.shape[0] != 4:
        raise ValueError("a shading mesh is a uint16 array of shape (4, mh, mw) in Q12 -- utils.raw_shading makes one of float gains --, "
                         "got %s %r" % (m.dtype, m.shape))
    if not all(_MESH_MIN <= n <= _MESH_MAX for n in m.shape[1:]):
        raise ValueError("a shading mesh has %d .. %d nodes a side, got %d x %d" % (_MESH_MIN, _MESH_MAX, m.shape[2], m.shape[1]))
    b = np.asarray(black)
    if b.shape != (4,) or b.dtype.kind not in "iu":
        raise ValueError("the black values of a shading map are four integers, got %s %r" % (b.dtype, b.shape))
    smax = (1 << bits) - 1
    if b.min() < 0 or b.max() > smax:
        raise ValueError("the black values of a shading map for %d-bit samples lie in 0 .. %d, got %r" % (bits, smax, b.tolist()))
    return RawShading(np.ascontiguousarray(m), b.astype(np.int32))


def raw_shading(gains, black_level=0, bits=8):
    """A lens-shading map for raw Bayer input (`LaneTracker(..., raw_shading=...)`): `gains` is a float mesh (mh, mw) -- one gain for all
    four colour phases -- or (4, mh, mw) -- a plane per phase: R, Gr, Gb, B --, 2 <= mh, mw <= 64, each gain in [0, 16), rounded to Q12:
    rint(4096 g).  `black_level` is the sensor's pedestal, one integer or four (per phase), 0 .. 2**bits - 1, bits = 8, 10 or 12: the gain
    acts on s - black and the pedestal stays in place, so a `raw_lut` built with the same black level follows unchanged.  A radial or
    polynomial model is sampled into a mesh by the caller.  ValueError for a gain outside [0, 16) or not a number, another shape, or a
    black level outside the samples' range.  -> RawShading(mesh uint16 (4, mh, mw), black int32 (4,))."""
    if bits not in (8, 10, 12):
        raise ValueError("bits is 8, 10 or 12, got %r" % (bits,))
    g = np.asarray(gains, dtype=np.float64)
    if g.ndim == 2:
        g = np.broadcast_to(g, (4,) + g.shape)
    if g.ndim != 3 or g.shape[0] != 4 or not all(_MESH_MIN <= n <= _MESH_MAX for n in g.shape[1:]):
        raise ValueError("shading gains are a mesh (mh, mw) or (4, mh, mw) with %d .. %d nodes a side, got %r" % (_MESH_MIN, _MESH_MAX, np.shape(gains)))
    if not np.all(np.isfinite(g)) or g.min() < 0 or not g.max() < 16:
        raise ValueError("shading gains lie in [0, 16), got %r .. %r" % (float(np.nanmin(g)) if g.size else None, float(np.nanmax(g)) if g.size else None))
    q = np.minimum(np.rint(4096.0 * g), 65535.0).astype(np.uint16)     # (15.9999 would round to 2^16)
    b = np.asarray(black_level)
    if b.dtype.kind not in "iu" or b.shape not in ((), (4,)):
        raise ValueError("black_level is one integer or four (R, Gr, Gb, B), got %r" % (black_level,))
    b = np.broadcast_to(b, (4,)).astype(np.int64)
    if b.min() < 0 or b.max() > (1 << bits) - 1:
        raise ValueError("black_level of %d-bit samples lies in 0 .. %d, got %r" % (bits, (1 << bits) - 1, black_level))
    return RawShading(np.ascontiguousarray(q), b.astype(np.int32))


def _mesh_nodes(n, m):
    """One axis of the expansion: n samples under m nodes -> (node in front of each sample, weight 0 .. 256 of the next one), int64."""
    u = np.arange(n, dtype=np.int64) * (m - 1) * 256 // (n - 1)
    i = np.minimum(u >> 8, m - 2)
    return i, u - (i << 8)


def raw_shading_plane(shading, pattern, img_size):
    """The gain of every site of an image of `img_size` = (W, H) with `pattern` under `shading`: uint16 (H, W), Q12.  With the mesh m of
    the site's phase p,

        u = x * (mw - 1) * 256 // (W - 1);  j = min(u >> 8, mw - 2);  a = u - (j << 8)
        v = y * (mh - 1) * 256 // (H - 1);  i = min(v >> 8, mh - 2);  b = v - (i << 8)
        G = ((256-a)*(256-b)*m[i][j] + a*(256-b)*m[i][j+1] + (256-a)*b*m[i+1][j] + a*b*m[i+1][j+1] + 32768) >> 16

    NumPy only.  This is the definition of what the device expands the mesh into."""
    p, bits, _ = _pattern_bits(pattern.replace("p_", "_", 1) if pattern in _BAYER_PACKED_PATTERNS else pattern)
    mesh, _black = checked_raw_shading(shading, bits)
    w, h = int(img_size[0]), int(img_size[1])
    if w < 2 or h < 2:
        raise ValueError("img_size is (width, height), both at least 2, got %r" % (img_size,))
    mh, mw = mesh.shape[1:]
    (j, a), (i, b) = _mesh_nodes(w, mw), _mesh_nodes(h, mh)
    i, b, j, a = i[:, None], b[:, None], j[None, :], a[None, :]
    out = np.empty((h, w), np.uint16)
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    phase = 2 * ((yy ^ (p >> 1)) & 1) + ((xx ^ (p & 1)) & 1)
    for ph in range(4):
        m = mesh[ph].astype(np.int64)
        g = ((256 - a) * (256 - b) * m[i, j] + a * (256 - b) * m[i, j + 1] + (256 - a) * b * m[i + 1, j] + a * b * m[i + 1, j + 1] + 32768) >> 16
        out[phase == ph] = g[phase == ph]
    return out


def apply_raw_shading(frames, pattern, shading):
    """Raw Bayer frames -- (H, W) or a stack (n, H, W); u8 for 'bayer_*', uint16 for 'bayer10_*' / 'bayer12_*' -- with the lens shading
    corrected: with G = `raw_shading_plane(shading, pattern, (W, H))`, B the black value of the site's phase, s the sample (a word masked
    to its bits) and smax = 2**bits - 1,

        s' = min(max(B + (((s - B) * G + 2048) >> 12), 0), smax)          int32, arithmetic shift (floor)

    in the frames' dtype.  NumPy only.  This is the definition: a raw Bayer tracker with `raw_shading=S` fed frames F computes, bit for
    bit, what the same tracker without a map computes from `apply_raw_shading(F, pattern, S)`."""
    p, bits, dtype = _pattern_bits(pattern)
    mesh, black = checked_raw_shading(shading, bits)
    a = np.asarray(frames)
    if a.dtype != dtype or a.ndim not in (2, 3):
        raise ValueError("%s frames are %s arrays (H, W) or (n, H, W), got %s %r" % (pattern, np.dtype(dtype), a.dtype, a.shape))
    h, w = a.shape[-2:]
    gain = raw_shading_plane(RawShading(mesh, black), pattern, (w, h)).astype(np.int64)
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    b = black.astype(np.int64)[2 * ((yy ^ (p >> 1)) & 1) + ((xx ^ (p & 1)) & 1)]
    smax = (1 << bits) - 1
    s = a.astype(np.int64) & smax
    return np.clip(b + (((s - b) * gain + 2048) >> 12), 0, smax).astype(dtype)


RawStats = collections.namedtuple("RawStats", "hist zone_count zone_sum rows cols")
RawStats.__doc__ = """Raw Bayer statistics (`utils.raw_stats`, `LaneTracker.raw_stats`): `hist` uint32 (4, bins) -- per colour phase (0 red sites, 1
green on red rows, 2 green on blue rows, 3 blue sites) the number of sites of the rectangle with each sample value --, `zone_count` uint32
(grid_h, grid_w) -- the valid 2 x 2 cells of each zone --, `zone_sum` uint64 (grid_h, grid_w, 4) -- the per-phase sums of their samples --,
each with a leading frame axis for a stack; `rows` = (row0, row1) and `cols` = (col0, col1), the rectangle they were taken of."""
_GRID_MAX = 64


def _raw_stats_format(pixel_format):
    """-> (the 16-bit or 8-bit format the samples are in once unpacked, pattern p, bits) of one of the twelve raw formats."""
    fmt = pixel_format.replace("p_", "_", 1) if pixel_format in _BAYER_PACKED_PATTERNS else pixel_format
    p, bits, _ = _pattern_bits(fmt)
    return fmt, p, bits


def checked_raw_stats_args(img_size, bits, default_rows, grid=(8, 8), rows=None, cols=None, lo=None, hi=None):
    """The arguments of a statistics call over frames of `img_size` = (W, H) with `bits`-bit samples, checked and filled in:
    -> ((row0, row1), (col0, col1), (grid_h, grid_w), lo int32 (4,), hi int32 (4,)).  rows=None: `default_rows`; cols=None: (0, W); lo / hi: one
    integer or four (by phase), None: 0 / 2**bits - 1.  ValueError for odd, empty or out-of-frame bounds, a grid side outside 1 .. 64 or above
    the rectangle's cells, a bound outside 0 .. 2**bits - 1."""
    w, h = int(img_size[0]), int(img_size[1])
    smax = (1 << bits) - 1

    def span(v, default, n, what):
        if v is None:
            v = default
        try:
            a, b = (int(t) for t in v)
            exact = all(int(t) == t for t in v)
        except (TypeError, ValueError):
            raise ValueError("%s is a pair of integers, got %r" % (what, v)) from None
        if not exact or a % 2 or b % 2 or not 0 <= a < b <= n:
            raise ValueError("%s = %r: both bounds are even, 0 <= first < last <= %d" % (what, tuple(v), n))
        return a, b
    r, c = span(rows, default_rows, h, "rows"), span(cols, (0, w), w, "cols")
    ncy, ncx = (r[1] - r[0]) // 2, (c[1] - c[0]) // 2
    try:
        gh, gw = (int(t) for t in grid)
        exact = all(int(t) == t for t in grid)
    except (TypeError, ValueError):
        raise ValueError("grid is (grid_h, grid_w), got %r" % (grid,)) from None
    if not exact or not (1 <= gh <= min(_GRID_MAX, ncy) and 1 <= gw <= min(_GRID_MAX, ncx)):
        raise ValueError("grid = %r: each side is 1 .. %d and at most the rectangle's cells, %d x %d (rows x columns)" % (tuple(grid), _GRID_MAX, ncy, ncx))

    def bounds(v, default, what):
        b = np.asarray(default if v is None else v)
        if b.dtype.kind not in "iu" or b.shape not in ((), (4,)):
            raise ValueError("%s is one integer or four (R, Gr, Gb, B), got %r" % (what, v))
        b = np.broadcast_to(b, (4,)).astype(np.int64)
        if b.min() < 0 or b.max() > smax:
            raise ValueError("%s of %d-bit samples lies in 0 .. %d, got %r" % (what, bits, smax, v))
        return b.astype(np.int32)
    return r, c, (gh, gw), bounds(lo, 0, "lo"), bounds(hi, smax, "hi")


def raw_stats(frames, pixel_format, grid=(8, 8), rows=None, cols=None, lo=None, hi=None, shading=None):
    """Statistics of raw Bayer frames -- one frame or a stack, in any of the twelve raw formats (u8 (H, W) for 'bayer_*', uint16 for 'bayer10_*' /
    'bayer12_*', u8 packed rows for 'bayer10p_*' / 'bayer12p_*') -- of the samples AS THEY ENTER THE RAW TABLE: the byte, the word masked to its
    bits, the unpacked sample (`unpack_raw`); with `shading` (a `utils.RawShading`) that sample taken through `apply_raw_shading`.  Table,
    demosaic and colour stage play no part: white-balance gains live in the table, so this is where an auto-white-balance loop measures.

    The rectangle: rows [row0, row1), columns [col0, col1), all even (None: the whole frame -- a tracker's `raw_stats` defaults to the rows its
    uploads bring), tiled by 2 x 2 cells anchored at even coordinates: ncy = (row1 - row0) // 2 by ncx = (col1 - col0) // 2 cells, each with one
    site of every phase p (0 R, 1 Gr, 2 Gb, 3 B: `apply_raw_lut`'s).  With smax = 2**bits - 1 and bins = 256 / 2**bits:

        hist[p][v]        uint32 (4, bins): the sites of phase p in the rectangle whose sample is v; every site counts
        zone of a cell    (cy * grid_h // ncy, cx * grid_w // ncx), `grid` = (grid_h, grid_w), 1 <= grid_h <= min(64, ncy), likewise grid_w
        a cell is valid   when all four of its samples satisfy lo[p] <= s_p <= hi[p] (one integer or four; None: 0 / smax; lo > hi: no cell)
        zone_count        uint32 (grid_h, grid_w): the valid cells of the zone
        zone_sum          uint64 (grid_h, grid_w, 4): the per-phase sums of the samples of the zone's valid cells

    -> RawStats(hist, zone_count, zone_sum, rows, cols), the arrays with a leading frame axis for a stack.  NumPy only.  This is the definition:
    `Context.raw_stats` / `LaneTracker.raw_stats` compute the same on the device, bit for bit."""
    fmt, p, bits = _raw_stats_format(pixel_format)
    a = unpack_raw(frames, pixel_format) if pixel_format in _BAYER_PACKED_PATTERNS else np.asarray(frames)
    dtype = np.uint8 if bits == 8 else np.uint16
    if a.dtype != dtype or a.ndim not in (2, 3):
        raise ValueError("%s frames are %s arrays (H, W) or (n, H, W), got %s %r" % (pixel_format, np.dtype(dtype), a.dtype, a.shape))
    h, w = a.shape[-2:]
    if h % 2 or w % 2 or h < 2 or w < 2:
        raise ValueError("a raw Bayer frame has an even height and width, got %r" % (a.shape,))
    smax, bins = (1 << bits) - 1, 1 << bits
    (row0, row1), (col0, col1), (gh, gw), lo, hi = checked_raw_stats_args((w, h), bits, (0, h), grid, rows, cols, lo, hi)
    s = (apply_raw_shading(a, fmt, shading) if shading is not None else a).astype(np.int64) & smax
    s = s.reshape((-1, h, w))[:, row0:row1, col0:col1]
    n, ncy, ncx = s.shape[0], (row1 - row0) // 2, (col1 - col0) // 2
    hist = np.zeros((n, 4, bins), np.uint32)
    site, valid = [None] * 4, np.ones((n, ncy, ncx), bool)
    for py in range(2):
        for px in range(2):
            ph = 2 * (py ^ (p >> 1)) + (px ^ (p & 1))
            site[ph] = s[:, py::2, px::2]
            for k in range(n):
                hist[k, ph] = np.bincount(site[ph][k].ravel(), minlength=bins)
            valid &= (site[ph] >= int(lo[ph])) & (site[ph] <= int(hi[ph]))
    # the zones are runs of consecutive cells along each axis, none empty (grid <= cells): sums over runs, in integers
    y0 = np.searchsorted(np.arange(ncy) * gh // ncy, np.arange(gh))
    x0 = np.searchsorted(np.arange(ncx) * gw // ncx, np.arange(gw))
    over_zones = lambda v: np.add.reduceat(np.add.reduceat(v.astype(np.uint64), y0, axis=1), x0, axis=2)
    zone_count = over_zones(valid).astype(np.uint32)
    zone_sum = np.stack([over_zones(np.where(valid, site[ph], 0)) for ph in range(4)], axis=-1)
    if a.ndim == 2:
        hist, zone_count, zone_sum = hist[0], zone_count[0], zone_sum[0]
    return RawStats(hist, zone_count, zone_sum, (row0, row1), (col0, col1))


def awb_gains(stats, black_level=0):
    """The grey-world step that closes the loop: the white-balance gains (R, G, B) that make the means of `stats` (a RawStats, of one frame or a
    stack: all valid cells of all frames count) grey.  With the pedestal `black_level` -- one integer or four (R, Gr, Gb, B) --, per phase
    m_p = sum_p / count - black_p and g = (m_1 + m_2) / 2: -> (g / m_0, 1.0, g / m_3), floats: the `gains=` argument of `utils.raw_lut`.
    ValueError when no cell is valid or a mean is not above the pedestal."""
    b = np.asarray(black_level)
    if b.dtype.kind not in "iu" or b.shape not in ((), (4,)):
        raise ValueError("black_level is one integer or four (R, Gr, Gb, B), got %r" % (black_level,))
    black = [int(v) for v in np.broadcast_to(b, (4,))]
    count = int(np.asarray(stats.zone_count, np.uint64).sum())
    if count == 0:
        raise ValueError("no valid cell: the statistics hold no sample to balance on")
    sums = [int(v) for v in np.asarray(stats.zone_sum, np.uint64).reshape(-1, 4).sum(axis=0)]
    m = [sums[p] / count - black[p] for p in range(4)]
    if min(m) <= 0:
        raise ValueError("a colour's mean is not above its black level: means %r over black %r" % ([sums[p] / count for p in range(4)], black))
    g = (m[1] + m[2]) / 2
    return (g / m[0], 1.0, g / m[3])


def bayer_to_rgb_color(frame, pattern, raw_lut=None, ccm=None, curve=None, shading=None):
    """A raw Bayer frame (H, W) or a stack (n, H, W) in any of the raw patterns -- u8 for 'bayer_*', uint16 for 'bayer10_*' /
    'bayer12_*', u8 packed rows (H, W * 5 // 4) / (H, W * 3 // 2) for 'bayer10p_*' / 'bayer12p_*' -- to RGB with the colour stage, on the device: every sample looked up in `raw_lut` (8-bit: u8 (4, 256), None: no
    table; 10 / 12 bits: u8 (4, 2**bits), None: the default), demosaiced, then `apply_raw_color(.., ccm, curve)`.  What a
    `LaneTracker(..., pixel_format=pattern, raw_lut=.., raw_ccm=.., raw_curve=..)` sees of the frame.  `shading`: a `utils.RawShading`
    applied to every sample first (`apply_raw_shading`), as `raw_shading=` of a tracker; with one and neither `ccm` nor `curve` there is
    no colour stage."""
    from . import _native
    from .lane_tracker import _context_for_module_functions
    if pattern not in _native.RAW_FORMATS:
        raise ValueError("pattern must be one of %s, got %r" % (", ".join(repr(n) for n in _native.RAW_FORMATS), pattern))
    raw_lut = _native.checked_raw_lut(raw_lut, pattern)
    ccm = None if ccm is None else checked_raw_ccm(ccm)
    curve = None if curve is None else checked_raw_curve(curve)
    shading = _native.checked_raw_shading(shading, pattern)
    a = _native.frames_array(frame, pattern)
    if a.ndim not in (2, 3):
        raise ValueError("a raw Bayer frame is an array (H, W), a stack of them (n, H, W); got %r" % (a.shape,))
    _native.raw_frame_size(np.empty(a.shape[-2:], a.dtype), pattern)       # (a size no raw frame has: refused before a context is made)
    ctx = _context_for_module_functions()
    convert = (lambda f: ctx.raw_to_rgb_color(f, pattern, raw_lut, ccm, curve)) if shading is None else \
              (lambda f: ctx.raw_to_rgb_shaded(f, pattern, shading, raw_lut, ccm, curve))
    if a.ndim == 2:
        return convert(a)
    if a.shape[0] == 0:
        return np.empty((0,) + _native.raw_frame_size(np.empty(a.shape[1:], a.dtype), pattern) + (3,), np.uint8)
    return np.stack([convert(a[k]) for k in range(a.shape[0])])


def rgb_to_yuv(frame, layout='nv12', matrix='bt601'):
    """The counterpart of `yuv_to_rgb`: an RGB frame (H, W, 3), H and W even, to YUV 4:2:0 as OpenCV holds it -- a u8 array
    (H * 3 // 2, W): the Y plane, then interleaved U,V rows ('nv12') or the U plane and the V plane ('i420') -- on the device,
    with OpenCV's integer arithmetic (`cv2.cvtColor(frame, cv2.COLOR_RGB2YUV_I420)`: chroma of the top-left pixel of each 2 x 2
    block, 20-bit fixed point; matrix='bt601': OpenCV's constants, video range; 'bt709' or eight integers {CRY, CGY, CBY, CRU, CGU,
    CBU, CGV, CBV} for another matrix).  What a device sink in that layout receives of an annotated frame."""
    from . import _native
    from .device import DeviceBuffer, DeviceFrames
    a = np.ascontiguousarray(frame, np.uint8)
    if _native.sink_format_id(layout) not in (1, 2):     # (packed 4:2:2 is an input format only: ValueError)
        raise ValueError("layout must be 'nv12' or 'i420'")
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] % 2 or a.shape[1] % 2 or 0 in a.shape:
        raise ValueError("an RGB frame is an array (H, W, 3) with H and W even, got %r" % (a.shape,))
    size = (a.shape[1], a.shape[0])
    k = _native.rgb2yuv_coeffs(matrix)
    with DeviceBuffer(a.nbytes) as src:
        src.copy_from_host(a)
        sink = DeviceFrames.empty(1, size, layout)
        try:
            _native.rgb_to_surfaces(src.ptr, a.nbytes, size, sink, k)
            return sink.to_host()[0]
        finally:
            sink.owner.close()



_RGB_ORDER = {"rgb": (0, 1, 2), "bgr": (2, 1, 0), "rgba": (0, 1, 2), "bgra": (2, 1, 0)}


def packed_to_rgb(frame, pixel_format):
    """A frame (or frames) of the RGB family -- 'bgr' (..., H, W, 3), 'rgba' / 'bgra' (..., H, W, 4); 'rgb' as it is -- as RGB
    (..., H, W, 3): a channel permutation, the alpha byte dropped.  NumPy only; what a `LaneTracker(..., pixel_format=...)` sees of
    the frame, bit for bit."""
    if pixel_format not in _RGB_ORDER:
        raise ValueError("pixel_format must be 'rgb', 'bgr', 'rgba' or 'bgra', got %r" % (pixel_format,))
    a = np.asarray(frame)
    want = 4 if pixel_format in ("rgba", "bgra") else 3
    if a.dtype != np.uint8 or a.ndim < 3 or a.shape[-1] != want:
        raise ValueError("a %r frame is a uint8 array (..., H, W, %d), got %s %r" % (pixel_format, want, a.dtype, a.shape))
    return np.ascontiguousarray(a[..., list(_RGB_ORDER[pixel_format])])


def rgb_to_packed(rgb, pixel_format, alpha=255):
    """The way back: RGB frames (..., H, W, 3) in `pixel_format` -- 'bgr', or 'rgba' / 'bgra' with every alpha byte `alpha` (what a
    device sink in that format receives: 255).  NumPy only."""
    if pixel_format not in _RGB_ORDER:
        raise ValueError("pixel_format must be 'rgb', 'bgr', 'rgba' or 'bgra', got %r" % (pixel_format,))
    a = np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim < 3 or a.shape[-1] != 3:
        raise ValueError("an RGB frame is a uint8 array (..., H, W, 3), got %s %r" % (a.dtype, a.shape))
    nch = 4 if pixel_format in ("rgba", "bgra") else 3
    out = np.empty(a.shape[:-1] + (nch,), np.uint8)
    for ch, at in enumerate(_RGB_ORDER[pixel_format]):
        out[..., at] = a[..., ch]
    if nch == 4:
        out[..., 3] = alpha
    return out
