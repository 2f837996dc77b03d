"""Drawing into the caller's device surfaces, the parts a CPU can check.

  arithmetic  lane_tracker_amd/csrc/inplace_arith.h (with yuv_arith.h and sink_arith.h) compiled for the host
              (tests/inplace_arith_host.cpp): 2 x 2 blocks of noise -- 0, 255 and bytes outside video range among them -- against the
              NumPy restatement (tests/inplace_reference.py), bit for bit: the bytes, and which of them were replaced
  keywords    out="inplace" on a tracker whose context is a CPU stand-in: every combination that is refused is refused before a
              frame is touched"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import inplace_reference as IR
import sink_reference as S
import yuv_reference as R
from fake_context import FakeContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def ia(tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler")
    out = str(tmp_path_factory.mktemp("inplace_arith") / "libinplace_arith_host.so")
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"),
                           os.path.join(ROOT, "tests", "inplace_arith_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.ia_draw_blocks.argtypes = [C.c_void_p] * 5 + [C.c_size_t, C.c_float] + [C.c_void_p] * 6
    lib.ia_draw_blocks.restype = None
    lib.ia_draw_pixels.argtypes = [C.c_void_p] * 3 + [C.c_size_t, C.c_float, C.c_void_p]
    lib.ia_draw_pixels.restype = None
    return lib


def _blocks(n, seed):
    """Noise blocks; the first ones hold the extremes: all 0, all 255, Y below 16 and above 235 with chroma at both ends."""
    rng = np.random.default_rng(seed)
    y4 = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    u, v = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    y4[0], u[0], v[0] = 0, 0, 0
    y4[1], u[1], v[1] = 255, 255, 255
    y4[2], u[2], v[2] = (3, 250, 15, 236), 0, 255
    y4[3], u[3], v[3] = (16, 235, 128, 1), 255, 0
    # per pixel: nothing, lane only, text only, both; lane values and alphas over their whole range, 1 and 255 included
    lane = rng.integers(0, 256, (n, 4)).astype(np.int32) * (rng.random((n, 4)) < 0.5)
    ta = rng.integers(0, 256, (n, 4)).astype(np.int32) * (rng.random((n, 4)) < 0.5)
    lane[4], ta[4] = (1, 255, 0, 2), (0, 0, 0, 0)
    lane[5], ta[5] = (0, 0, 0, 0), (1, 255, 0, 128)
    lane[6], ta[6] = (0, 255, 255, 255), (0, 0, 255, 1)                   # an undrawn top-left: chroma stays
    return y4, u, v, np.ascontiguousarray(lane, np.int32), np.ascontiguousarray(ta, np.int32)


@pytest.mark.parametrize("matrices", [("bt601", "bt601"), ("bt709", "bt709"), ("bt601", S.CLAMPING)], ids=["bt601", "bt709", "clamping"])
def test_blocks_against_the_restatement(ia, matrices):
    in_matrix, out_matrix = matrices
    n = 200000
    y4, u, v, lane, ta = _blocks(n, 17)
    kin = np.array(R.MATRICES[in_matrix], np.int32)
    kout = np.array(S.coeffs(out_matrix), np.int32)
    yo, uo, vo, ch = np.empty_like(y4), np.empty_like(u), np.empty_like(v), np.empty(n, np.uint8)
    ia.ia_draw_blocks(y4.ctypes.data, u.ctypes.data, v.ctypes.data, lane.ctypes.data, ta.ctypes.data, n, 0.3, kin.ctypes.data, kout.ctypes.data,
                      yo.ctypes.data, uo.ctypes.data, vo.ctypes.data, ch.ctypes.data)
    wy, wu, wv, changed = IR.block_expected(y4, u, v, lane, ta, in_matrix, out_matrix)
    assert np.array_equal(yo, wy) and np.array_equal(uo, wu) and np.array_equal(vo, wv)
    bits = (ch[:, None] >> np.arange(4)) & 1
    assert np.array_equal(bits.astype(bool), changed) and np.array_equal((ch >> 4) & 1, changed[:, 0])
    # what was not drawn on keeps its bytes -- and those are not the round trip's
    untouched = ~changed
    assert np.array_equal(yo[untouched], y4[untouched]) and np.array_equal(uo[~changed[:, 0]], u[~changed[:, 0]])
    assert untouched.any() and changed.any() and 0 < changed[:, 0].mean() < 1
    # a lane value or an alpha does not always change the pixel (a saturated green, 0.3 * 1 rounds away): then nothing is replaced
    assert ((lane != 0) & ~changed & (ta == 0)).any()


def test_pixels_against_the_restatement(ia):
    rng = np.random.default_rng(3)
    n = 300000
    px = rng.integers(0, 1 << 24, n).astype(np.uint32)
    lane = (rng.integers(0, 256, n) * (rng.random(n) < 0.6)).astype(np.int32)
    ta = (rng.integers(0, 256, n) * (rng.random(n) < 0.6)).astype(np.int32)
    out = np.empty_like(px)
    ia.ia_draw_pixels(px.ctypes.data, lane.ctypes.data, ta.ctypes.data, n, 0.3, out.ctypes.data)
    c = np.stack([px & 255, (px >> 8) & 255, (px >> 16) & 255], -1).astype(np.int64)
    g = c[:, 1].astype(np.float32) + (lane.astype(np.float32) * np.float32(0.3)).astype(np.float32)
    c[:, 1] = np.where(lane != 0, np.clip(np.rint(g), 0, 255).astype(np.int64), c[:, 1])
    c = np.where((ta != 0)[:, None], c + ((255 - c) * ta[:, None].astype(np.int64) + 127) // 255, c)
    assert np.array_equal(out, (c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)).astype(np.uint32))


def test_the_round_trip_is_not_the_identity():
    """The reason the in-place form keeps the decoder's bytes: on noise the whole-frame conversion changes most of them."""
    f = np.random.default_rng(0).integers(0, 256, (48 * 3 // 2, 64), dtype=np.uint8)
    for layout in ("nv12", "i420"):
        assert (IR.round_trip(f, layout) != f).mean() > 0.5
        same, changed = IR.expected(f, R.yuv420_to_rgb(f, layout), layout)
        assert np.array_equal(same, f) and not changed.any()              # nothing drawn: nothing replaced


# ---- keywords ---------------------------------------------------------------------------------------------------------------------------
class _Ctx(FakeContext):
    """The stand-in with the few calls a DeviceFrames window makes before its first frame is touched."""

    def attach_device_frames(self, frames, first=0):
        raise AssertionError("a frame was touched")

    def upload_frame_rows_async(self, frames, first=0):
        raise AssertionError("a frame was touched")

    def set_input_format(self, pixel_format, matrix="bt601"):
        pass


def _tracker(monkeypatch, **kw):
    from lane_tracker_amd import _native, calib
    from lane_tracker_amd import lane_tracker as LT
    monkeypatch.setattr(_native, "Context", _Ctx)
    cal = calib.reference_calibration()
    return LT.LaneTracker(**cal, **kw), cal


def _device_frames(cal, layout="rgb", n=2, **kw):
    from lane_tracker_amd import _native
    from lane_tracker_amd.device import DeviceFrames
    w, h = cal["img_size"]
    surf = np.zeros(n, _native.SURFACE_DTYPE)
    surf["plane"][:, :3] = 0x10000                                       # (never dereferenced: every call here is refused first)
    surf["pitch"], surf["chroma_pitch"] = (3 * w if layout == "rgb" else w), (0 if layout == "rgb" else w)
    return DeviceFrames(surf, (w, h), layout, **kw)


def test_keywords_refused_before_a_frame_is_touched(monkeypatch):
    from lane_tracker_amd.device import DeviceFrames
    t, cal = _tracker(monkeypatch)
    w, h = cal["img_size"]
    feed = _device_frames(cal)
    host = np.zeros((2, h, w, 3), np.uint8)
    calls = [dict(frames=host, out="inplace"),                                        # host arrays: annotate="inplace" is theirs
             dict(frames=feed, out="inplace", annotate=False),
             dict(frames=feed, out="inplace", annotate="inplace"),
             dict(frames=feed, out="inplace", visualize_search=True),
             dict(frames=feed, out="inplace", split_view=True),
             dict(frames=feed, out="somewhere"),                                      # no such destination
             dict(frames=feed, out="inplace", out_yuv_matrix="bt2020"),               # no such matrix
             dict(frames=_device_frames(cal, readonly=True), out="inplace"),          # a read-only source
             dict(frames=feed[0:1], out="inplace", annotate=False),
             dict(frames=feed, annotate="inplace"),                                   # (as ever)
             dict(frames=feed, annotate="inplace", out=feed)]
    for kw in calls:
        kw = dict(kw)
        frames = kw.pop("frames")
        with pytest.raises(ValueError):
            t.process_batch(frames, **kw)
        with pytest.raises(ValueError):
            list(t.process_stream([frames], **kw))
    assert t.counter == 0
    # the message for host arrays points to the other spelling
    with pytest.raises(ValueError, match="annotate='inplace'"):
        t.process_batch(host, out="inplace")
    # a view of read-only frames is read-only
    ro = _device_frames(cal, readonly=True)
    assert ro[0].readonly and ro[0:1].readonly and not feed[0].readonly
    assert DeviceFrames.from_cuda_array({"shape": (h, w, 3), "typestr": "|u1", "data": (0x10000, True), "version": 3}).readonly
    assert not DeviceFrames.from_cuda_array({"shape": (h, w, 3), "typestr": "|u1", "data": (0x10000, False), "version": 3}).readonly


def test_the_matrix_of_the_way_back(monkeypatch):
    from lane_tracker_amd import _native
    t, cal = _tracker(monkeypatch, pixel_format="nv12", yuv_matrix="bt709")
    assert t._inplace_matrix("inplace", None) == "bt709"                  # the tracker's own, when it is a preset
    assert t._inplace_matrix("inplace", "bt601") == "bt601"
    custom, _ = _tracker(monkeypatch, pixel_format="nv12", yuv_matrix=_native.YUV_MATRICES["bt709"])
    feed = _device_frames(cal, "nv12")
    with pytest.raises(ValueError, match="out_yuv_matrix"):
        custom.process_batch(feed, out="inplace")                          # a custom input matrix names none
    with pytest.raises(ValueError, match="out_yuv_matrix"):
        list(custom.process_stream([feed], out="inplace"))
    assert custom._inplace_matrix("inplace", list(S.MATRICES["bt709"])) == list(S.MATRICES["bt709"])
    assert custom.counter == 0
    rgb, _ = _tracker(monkeypatch)
    assert rgb._inplace_matrix("inplace", None) == "bt601"                # (an RGB tracker: not read)
