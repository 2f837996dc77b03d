"""The front end's matrix: (pixel format x source x table form x range shape) -> undistorted rows, R plane, Lab-b plane, against the
CPU oracle.  This module builds the cases and the reference and needs no GPU (test_front_matrix_cpu.py holds the inputs to what they
are for; test_gpu_front_matrix.py runs them).

Sizes (camera = bird's-eye size): A 64 x 48 (width a multiple of 4: k_warp_split4 / k_warp_cal<4>), B 66 x 50 (24-bit rows of 198
bytes and a bird's-eye width that are no multiples of 4: k_warp_split1 / k_warp_cal<1>), C 37 x 21 (odd in both directions, frames
2331 bytes apart: the unaligned forms of plain RGB; the RGB family only -- the YUV and raw Bayer formats need even sizes).

Four calibration sets per size: the identity (every row and column, so the rows of a context are the whole image), one with taps
outside the image in both remaps, one whose bird's-eye view reads a narrow run of camera rows, one with a general affine view.

The reference of a slot: its frame to RGB per source pixel (the walk converts before it blends), then the oracle with the slot's
set: undistort(), front_end()[..., 0], lab_b(front_end())."""
import functools

import numpy as np

import bayer_reference as RB
import yuv422_reference as R422
import yuv_reference as R420

SIZES = {"A": (64, 48), "B": (66, 50), "C": (37, 21)}
FORMATS = ("rgb", "nv12", "i420", "yuy2", "uyvy", "bgr", "rgba", "bgra") + RB.PATTERNS
RGB_FAMILY = ("rgb", "bgr", "rgba", "bgra")
BPP = {"rgb": 3, "bgr": 3, "rgba": 4, "bgra": 4}
N_SETS = 4
CAPACITY = 72
FILL = 0xEE
FIRSTS = (1, 3)                          # the first slots of the mixed ranges (rows 3 and 4 of the GPU test's table)


def formats_of(size):
    return RGB_FAMILY if size == "C" else FORMATS


def cases():
    """(format, size) of every context of the matrix."""
    return [(f, s) for s in SIZES for f in formats_of(s)]


def yuv_matrix(size):
    return "bt709" if size == "B" else "bt601"


def calibration_sets(size):
    """The four sets of a size, set 0 first.  At size C the calibrations shrink with the image -- the translations of the bird's-eye
    matrices and the focal lengths, by W / 64 and H / 48 -- so that every set still reads a run of camera rows, set 2's stays inside
    the image, and set 1 keeps its share of taps outside the image (with the focal lengths of the larger sizes 5 % of its taps
    would lie fully outside; test_front_matrix_cpu.py asks for 10 % at every size)."""
    w, h = SIZES[size]
    cx, cy = (w - 1) / 2, (h - 1) / 2
    sx, sy = (w / 64, h / 48) if size == "C" else (1.0, 1.0)
    K = lambda fx, fy, x, y: np.array([[fx * sx, 0, x], [0, fy * sy, y], [0, 0, 1.0]])
    M = lambda a, b, tx, c, d, ty: np.array([[a, b, tx * sx], [c, d, ty * sy], [0, 0, 1.0]])
    return [dict(cam_matrix=np.eye(3), dist_coeffs=np.zeros(5), M=np.eye(3)),
            dict(cam_matrix=K(40, 40, cx, cy), dist_coeffs=np.array([0.3, 0, 0.01, 0, 0]), M=M(1, 0, -9.5, 0, 1, 6.25)),
            dict(cam_matrix=K(55, 50, cx + 2, cy - 1), dist_coeffs=np.array([-0.2, 0.05, 0, 0.01, 0]), M=M(1, 0, 0, 0, 2, -30.5)),
            dict(cam_matrix=K(48, 48, cx - 3, cy + 2), dist_coeffs=np.array([0.1, 0, 0, 0, 0]), M=M(1.1, 0.05, -4.25, 0.02, 1.2, -3.5))]


def ids_pattern(n):
    """The sets of the slots of a mixed range, by index in the range."""
    return [(i + i // 5) % N_SETS for i in range(n)]


def alternating_runs(n):
    """[(a, b, attached)]: runs of lengths 1, 2, 3, 1, 2, 3, ... over the indices 0 .. n - 1, attached and plain in turn (the first
    attached)."""
    out, a, k = [], 0, 0
    while a < n:
        b = min(n, a + 1 + k % 3)
        out.append((a, b, k % 2 == 0))
        a, k = b, k + 1
    return out


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def frame_shape(fmt, size):
    w, h = SIZES[size]
    if fmt in BPP:
        return (h, w, BPP[fmt])
    if fmt in RB.PATTERNS:
        return (h, w)
    return (h, w, 2) if fmt in R422.ORDERS else (h * 3 // 2, w)


def case_seed(fmt, size):
    return 1000 + 16 * "ABC".index(size) + FORMATS.index(fmt)


@functools.lru_cache(maxsize=None)
def frame_pool(fmt, size, n=CAPACITY):
    """n frames of uniform noise in the format's own layout (alpha bytes included), seeded by the case; shared, never changed."""
    out = np.random.default_rng(case_seed(fmt, size)).integers(0, 256, (n,) + frame_shape(fmt, size), dtype=np.uint8)
    out.setflags(write=False)
    return out


def to_rgb(frames, fmt, matrix="bt601"):
    """One frame or a stack of frames in `fmt` -> RGB, per pixel: the definitions the per-format suites hold the kernels to."""
    f = np.asarray(frames)
    if fmt in BPP:
        pick = {"rgb": lambda a: a, "bgr": lambda a: a[..., ::-1], "rgba": lambda a: a[..., :3], "bgra": lambda a: a[..., 2::-1]}[fmt]
        return np.ascontiguousarray(pick(f))
    if fmt in RB.PATTERNS:
        return RB.bayer_to_rgb(f, fmt)
    one = (lambda a: R422.yuv422_to_rgb(a, fmt, matrix)) if fmt in R422.ORDERS else (lambda a: R420.yuv420_to_rgb(a, fmt, matrix))
    nd = 3 if fmt in R422.ORDERS else 2
    return one(f) if f.ndim == nd else np.stack([one(a) for a in f])


@functools.lru_cache(maxsize=None)
def rgb_pool(fmt, size):
    out = to_rgb(frame_pool(fmt, size), fmt, yuv_matrix(size))
    out.setflags(write=False)
    return out


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


@functools.lru_cache(maxsize=None)
def oracle_calib(size, s):
    c = calibration_sets(size)[s]
    return _oracle().make_calib(SIZES[size], SIZES[size], c["cam_matrix"], c["dist_coeffs"], c["M"])


@functools.lru_cache(maxsize=None)
def source_rows(size, s):
    """Rows [r0, r1) of the undistorted image that the bird's-eye view of set s reads."""
    return _oracle().warp_source_rows(oracle_calib(size, s))


@functools.lru_cache(maxsize=None)
def reference(fmt, size, s, k):
    """Frame k of the case's pool through set s -> (undistorted image, R plane, Lab-b plane), once."""
    O, oc, rgb = _oracle(), oracle_calib(size, s), rgb_pool(fmt, size)[k]
    bev = O.front_end(oc, rgb)
    out = (O.undistort(oc, rgb), np.ascontiguousarray(bev[..., 0]), O.lab_b(bev))
    for a in out:
        a.setflags(write=False)
    return out


def tap_stats(size, s):
    """The undistortion taps of set s over the whole image -> fractions of pixels whose 2 x 2 taps lie (partly, fully) outside the
    image, and of pixels with a non-zero blend fraction."""
    w, h = SIZES[size]
    xy, frac = _oracle().undistort_map(oracle_calib(size, s))
    sx, sy = xy[..., 0].astype(int), xy[..., 1].astype(int)
    inx = [(sx + d >= 0) & (sx + d < w) for d in (0, 1)]
    iny = [(sy + d >= 0) & (sy + d < h) for d in (0, 1)]
    inside = sum((a & b).astype(int) for a in inx for b in iny)
    fx, fy = frac & 31, frac >> 5
    return float(((inside > 0) & (inside < 4)).mean()), float((inside == 0).mean()), float(((fx > 0) | (fy > 0)).mean())


# ---- surfaces ----------------------------------------------------------------------------------------------------------------------
def surface_pitches(fmt, size):
    """(pitch, chroma pitch or None): five bytes more than a row holds."""
    w, _ = SIZES[size]
    if fmt in BPP:
        return BPP[fmt] * w + 5, None
    if fmt in R422.ORDERS:
        return 2 * w + 5, None
    if fmt in RB.PATTERNS:
        return w + 5, None
    return w + 5, (w if fmt == "nv12" else w // 2) + 5


def pack_surfaces(frames, fmt, size, offset):
    """pack_host_frames at the matrix's pitches: the block (FILL between the rows, ending on the last byte of the last row) and the
    surfaces with plane offsets into it."""
    from lane_tracker_amd.device import pack_host_frames
    pitch, cp = surface_pitches(fmt, size)
    block, surf, img_size, _ = pack_host_frames(frames, fmt, pitch=pitch, chroma_pitch=cp, offset=offset, fill=FILL)
    assert img_size == SIZES[size]
    return block, surf


def device_surfaces(frames, fmt, size, offset):
    """The frames as pitched surfaces in a DeviceBuffer of their own (needs the GPU)."""
    from lane_tracker_amd.device import DeviceBuffer, DeviceFrames
    block, surf = pack_surfaces(frames, fmt, size, offset)
    buf = DeviceBuffer(block.nbytes).copy_from_host(block)
    surf["plane"][:, :{"nv12": 2, "i420": 3}.get(fmt, 1)] += np.uint64(buf.ptr)
    return DeviceFrames(surf, SIZES[size], fmt, owner=buf)
