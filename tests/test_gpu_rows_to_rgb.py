"""The row conversions behind a shown camera frame -- k_rows_to_rgb<LAYOUT, SURF, WIDE> -- through the entry points that show one: the
`rest` uploads (the slots' staging frames), lt_device_frames_rest (attached surfaces) and lt_yuv_to_rgb / lt_bayer_to_rgb, for every
layout, both sources and both launch rules, bit for bit against the NumPy definitions front_matrix.to_rgb and bayer_reference hold.

  16-column body  the width and every base and pitch of the launch multiples of 16: 32 x 8 (raw Bayer: 16 x 4, one thread owns the
                  frame's first and last column at once), dense frames
  byte-wise body  34 x 10 with dense frames; 32 x 8 on surfaces at pitch = row bytes + 5, offset 3

The rows: a run with an odd first row and an odd end, [3, 7), so that both halves of a 4:2:0 chroma pair fall outside once; for raw
Bayer the frame's first and last row, whose demosaic is their neighbour's.  Rows outside the runs keep the fill."""
import numpy as np
import pytest

import bayer_reference as RB
import front_matrix as FM
import yuv422_reference as R422
from lane_tracker_amd import _native
from lane_tracker_amd.device import DeviceBuffer, DeviceFrames, pack_host_frames

pytestmark = pytest.mark.gpu

FORMATS = [f for f in FM.FORMATS if f != "rgb"]             # (plain RGB rows are shown as they are)
N, FIRST = 3, 1


def _shape(fmt, w, h):
    if fmt in FM.BPP:
        return (h, w, FM.BPP[fmt])
    return (h, w) if fmt in RB.PATTERNS else (h, w, 2) if fmt in R422.ORDERS else (h * 3 // 2, w)


def _size(fmt, source, form):
    if form == "wide":
        return (16, 4) if fmt in RB.PATTERNS else (32, 8)
    return (34, 10) if source == "slots" else (32, 8)


def _runs(fmt, h):
    return (0, 1, h - 1, h) if fmt in RB.PATTERNS else (3, 7, 7, 7)


def _surfaces(frames, fmt, w, padded):
    """Dense, 16-byte aligned surfaces, or (padded) five bytes more than a row holds between the rows and the first plane at byte 3."""
    rb = frames.shape[2] * (frames.shape[3] if frames.ndim == 4 else 1)
    cp = {"nv12": w, "i420": w // 2}.get(fmt)
    kw = dict(pitch=rb + 5, chroma_pitch=None if cp is None else cp + 5, offset=3) if padded else {}
    block, surf, _, _ = pack_host_frames(frames, fmt, fill=FM.FILL, **kw)
    buf = DeviceBuffer(block.nbytes).copy_from_host(block)
    surf["plane"][:, :{"nv12": 2, "i420": 3}.get(fmt, 1)] += np.uint64(buf.ptr)
    bits = int(buf.ptr) | int(surf["pitch"][0]) | int(surf["chroma_pitch"][0]) | int(np.bitwise_or.reduce(surf["plane"].reshape(-1)))
    assert (bits & 15 != 0) == padded, "the surfaces take the %s body" % ("byte-wise" if padded else "16-column")
    return DeviceFrames(surf, (w, h_of(frames, fmt)), fmt, owner=buf)


def h_of(frames, fmt):
    return frames.shape[1] * 2 // 3 if fmt in ("nv12", "i420") else frames.shape[1]


def _read_back(c, h, w):
    """Every row of the camera frames of the slots, through the overlay with no points (a plain copy) over two runs that cover the frame."""
    e = np.zeros(0, np.int64)
    rows = np.array([0, h // 2, h // 2, h], np.int32)
    c.overlay_run([(e, e, e, e)] * N, first=FIRST, rows=rows.ctypes.data)
    out = _native.pinned_empty((N, h, w, 3))
    out[:] = 0
    c.download_overlay_async(out, first=FIRST, rows=rows.ctypes.data)
    c.sync()
    return np.array(out)


@pytest.mark.parametrize("form", ["wide", "bytewise"])
@pytest.mark.parametrize("source", ["slots", "surfaces"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_of_a_shown_frame_are_the_definition(fmt, source, form):
    w, h = _size(fmt, source, form)
    if source == "slots":                                    # (lt_api.cpp: the slots' frames lie h * w * 3 bytes apart)
        assert ((w & 15) == 0 and (h * w * 3) % 16 == 0) == (form == "wide")
    matrix = "bt709" if form == "wide" else "bt601"
    frames = np.random.default_rng(FM.FORMATS.index(fmt) * 4 + w).integers(0, 256, (N,) + _shape(fmt, w, h), dtype=np.uint8)
    fill = np.full_like(frames, FM.FILL)
    want, held = FM.to_rgb(frames, fmt, matrix), FM.to_rgb(fill, fmt, matrix)
    if fmt in FM.BPP or fmt in RB.PATTERNS:
        assert (held == FM.FILL).all()
    runs = _runs(fmt, h)
    rows = np.array(runs, np.int32)
    for lo, hi in (runs[:2], runs[2:]):
        held[:, lo:hi] = want[:, lo:hi]
    M = np.diag([64 / w, 48 / h, 1.0])                       # an identity camera: every row is read
    c = _native.Context((w, h), (64, 48), np.eye(3), np.zeros(5), M, capacity=N + 1)
    try:
        c.set_input_format(fmt, matrix)
        c.overlay_configure(np.linalg.inv(M))
        c.upload_frames(fill, first=FIRST)
        assert np.array_equal(_read_back(c, h, w), FM.to_rgb(fill, fmt, matrix)), "the fill"
        if source == "slots":
            keep = [c.upload_frame_rows(frames, first=FIRST, enqueue=True)]
            c.mask_run(N, first=FIRST)
            keep.append(c.upload_frame_rest(frames, first=FIRST, rows=rows.ctypes.data))
            got = _read_back(c, h, w)
        else:
            dev = _surfaces(frames, fmt, w, padded=form == "bytewise")
            try:
                keep = c.attach_device_frames(dev, first=FIRST)
                c.mask_run(N, first=FIRST)
                c.device_frames_rest(N, first=FIRST, rows=rows.ctypes.data)
                got = _read_back(c, h, w)
            finally:
                dev.owner.close()
        del keep
        assert np.array_equal(got, held), (fmt, source, form, np.argwhere(got != held)[:4])
    finally:
        c.close()


@pytest.mark.parametrize("form", ["wide", "bytewise"])
@pytest.mark.parametrize("fmt", [f for f in FORMATS if f not in FM.BPP])
def test_one_frame_to_rgb_is_the_definition(fmt, form):
    """lt_yuv_to_rgb / lt_bayer_to_rgb: a dense frame in fresh device memory, every row."""
    w, h = _size(fmt, "slots", form)
    matrix = "bt601" if form == "wide" else "bt709"
    frame = np.random.default_rng(FM.FORMATS.index(fmt) * 4 + h).integers(0, 256, _shape(fmt, w, h), dtype=np.uint8)
    c = _native.Context((64, 48), (64, 48), np.eye(3), np.zeros(5), np.eye(3), capacity=1)
    try:
        got = c.bayer_to_rgb(frame, fmt) if fmt in RB.PATTERNS else c.yuv_to_rgb(frame, fmt, matrix)
    finally:
        c.close()
    want = FM.to_rgb(frame, fmt, matrix)
    assert got.shape == (h, w, 3) and np.array_equal(got, want), (fmt, form, np.argwhere(got != want)[:4])
