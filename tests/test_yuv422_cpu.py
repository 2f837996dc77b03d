"""Packed YUV 4:2:2 input (YUY2 / UYVY) without a GPU: the NumPy restatement (`tests/yuv422_reference.py`) held against bytes written
out here, against the pinned 4:2:0 restatement and against OpenCV where it imports; the byte-position arithmetic of
`csrc/yuv_arith.h` compiled for the host and checked exhaustively (`tests/yuv422_arith_host.cpp`, once more under ASan + UBSan);
what `DeviceFrames` and a tracker accept and refuse before any device call; raw `.yuy2` / `.uyvy` files; the C header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import yuv422_reference as R422
import yuv_reference as R
from fake_context import FakeContext
from lane_tracker_amd import _native, video
from lane_tracker_amd.device import DeviceFrames, pack_host_frames
from test_yuv_cpu import TRIPLES

try:
    import cv2
except Exception:   # ImportError, or a broken binary wheel
    cv2 = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
LAYOUTS = ["yuy2", "uyvy"]
BASE = 0x7f0000001000          # a made-up device address: nothing here dereferences it


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("yuv,bt601,bt709", TRIPLES)
def test_written_out_macropixels(layout, yuv, bt601, bt709):
    """One macropixel written out byte by byte, both of its pixels; and beside a macropixel of another colour."""
    y, u, v = yuv
    mp = [y, u, y, v] if layout == "yuy2" else [u, y, v, y]
    other = [16, 128, 16, 128] if layout == "yuy2" else [128, 16, 128, 16]                 # black
    frame = np.array(mp + other, np.uint8).reshape(1, 4, 2)
    for matrix, want in (("bt601", bt601), ("bt709", bt709)):
        got = R422.yuv422_to_rgb(frame, layout, matrix)
        assert got.shape == (1, 4, 3)
        assert [tuple(int(c) for c in p) for p in got[0]] == [want, want, (0, 0, 0), (0, 0, 0)]
    # the two pixels of a macropixel share its chroma and differ in luma only
    lum = np.array([235, u, 16, v] if layout == "yuy2" else [u, 235, v, 16], np.uint8).reshape(1, 2, 2)
    a, b = R422.yuv422_to_rgb(lum, layout)[0]
    assert tuple(a) == tuple(int(c) for c in R.convert_triples(235, u, v)) and tuple(b) == tuple(int(c) for c in R.convert_triples(16, u, v))


def test_byte_orders_hold_the_same_picture():
    rgb = np.random.default_rng(4).integers(0, 256, (33, 66, 3), dtype=np.uint8)          # an odd height
    yuy2, uyvy = R422.rgb_to_yuv422(rgb, "yuy2"), R422.rgb_to_yuv422(rgb, "uyvy")
    assert yuy2.shape == uyvy.shape == (33, 66, 2) and not np.array_equal(yuy2, uyvy)
    assert np.array_equal(yuy2.reshape(33, 33, 4)[..., [1, 0, 3, 2]], uyvy.reshape(33, 33, 4))
    assert np.array_equal(R422.yuv422_to_rgb(yuy2, "yuy2"), R422.yuv422_to_rgb(uyvy, "uyvy"))
    flat = np.full((3, 8, 3), (200, 40, 90), np.uint8)                      # a flat colour survives the round trip to within rounding
    assert np.abs(R422.yuv422_to_rgb(R422.rgb_to_yuv422(flat, "uyvy"), "uyvy").astype(int) - flat).max() <= 2


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_equal_chroma_rows_convert_like_the_pinned_420_restatement(layout, matrix):
    """A 4:2:2 frame whose chroma rows are equal in pairs IS a 4:2:0 picture: exactly what yuv420_to_rgb gives for the NV12 frame
    with those chroma rows."""
    rng = np.random.default_rng(12)
    h, w = 10, 24
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u, v = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    f422 = R422.pack_422(y, np.repeat(u, 2, 0), np.repeat(v, 2, 0), layout)
    nv12 = np.concatenate([y.reshape(-1), np.stack([u, v], -1).reshape(-1)]).reshape(h * 3 // 2, w)
    want = R.yuv420_to_rgb(nv12, "nv12", matrix)
    assert np.array_equal(R422.yuv422_to_rgb(f422, layout, matrix), want)
    assert want.min() == 0 and want.max() == 255


@pytest.mark.skipif(cv2 is None, reason="UNVERIFIED vs OpenCV (cv2 absent)")
@pytest.mark.parametrize("layout", LAYOUTS)
def test_restatement_is_opencv(layout):
    frame = np.random.default_rng(9).integers(0, 256, (721, 1280, 2), dtype=np.uint8)
    code = cv2.COLOR_YUV2RGB_YUY2 if layout == "yuy2" else cv2.COLOR_YUV2RGB_UYVY
    assert np.array_equal(R422.yuv422_to_rgb(frame, layout, "bt601"), cv2.cvtColor(frame, code))


# ---- the position arithmetic of yuv_arith.h, on the host ------------------------------------------------------------------------
@pytest.mark.skipif(CXX is None, reason="no C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_position_arithmetic_exhaustively(tmp_path, flags):
    """Every even W in 4 .. 18, every cxl, both orders, both taps: window and bit positions select what direct indexing selects; the
    window starts inside its row and ends at 4 * min(cxl >> 1, W / 2 - 2) + 8 <= 2 W (rows are heap blocks of exactly 2 W bytes).
    2 orders x sum over W of (W - 1) x 2 taps x 8 rows = 2560 checks."""
    exe = str(tmp_path / "yuv422_arith_host")
    build = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"),
                            os.path.join(ROOT, "tests", "yuv422_arith_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert run.stdout.strip() == "ok 2560"


# ---- the Python surface, no device ------------------------------------------------------------------------------------------------
def _iface(shape, strides=None, ptr=BASE, **more):
    return dict({"shape": tuple(shape), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": strides}, **more)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_frame_shape_and_format_tables(layout):
    assert _native.frame_shape((64, 48), layout) == (48, 64, 2)
    assert _native.frame_shape((64, 47), layout) == (47, 64, 2)              # any height
    for size in ((63, 48), (2, 48), (0, 48)):
        with pytest.raises(ValueError):
            _native.frame_shape(size, layout)
    assert _native.pixel_format_id(layout) == {"yuy2": 3, "uyvy": 4}[layout] == _native.INPUT_FORMATS[layout]
    with pytest.raises(ValueError, match="input format only"):
        _native.sink_format_id(layout)
    assert [_native.sink_format_id(f) for f in ("rgb", "nv12", "i420")] == [0, 1, 2]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_device_frames_from_cuda_array_and_planes(layout):
    H, W = 5, 8
    for pitch in (2 * W, 2 * W + 5):
        one = DeviceFrames.from_cuda_array(_iface((H, W, 2), (pitch, 2, 1)), layout)
        assert one.single and len(one) == 1 and one.img_size == (W, H) and one.shape == (H, W, 2) and one.pixel_format == layout
        assert int(one.surfaces["plane"][0, 0]) == BASE and int(one.surfaces["pitch"][0]) == pitch and not one.surfaces["plane"][0, 1:].any()
        fs = H * pitch + 11
        many = DeviceFrames.from_cuda_array(_iface((3, H, W, 2), (fs, pitch, 2, 1)), layout)
        assert not many.single and many.shape == (3, H, W, 2)
        assert [int(p) for p in many.surfaces["plane"][:, 0]] == [BASE + k * fs for k in range(3)] and set(many.surfaces["pitch"]) == {pitch}
        assert many[1].single and int(many[1].surfaces["plane"][0, 0]) == BASE + fs
        p = DeviceFrames.from_planes([(BASE,), (BASE + fs,)], (W, H), layout, pitch=pitch)          # one plane, no chroma pitch
        assert len(p) == 2 and p.shape == (2, H, W, 2) and set(p.surfaces["pitch"]) == {pitch} and set(p.surfaces["chroma_pitch"]) == {0}
        assert DeviceFrames.from_planes((BASE,), (W, H), layout, pitch=pitch).single
    dense = DeviceFrames.from_cuda_array(_iface((2, H, W, 2)), layout)                             # no strides: C order
    assert set(dense.surfaces["pitch"]) == {2 * W} and int(dense.surfaces["plane"][1, 0]) == BASE + H * W * 2
    for bad in (_iface((H, W - 1, 2)),                         # an odd width
                _iface((H, 2, 2)),                             # one macropixel
                _iface((H, W, 3)), _iface((H, 2 * W)), _iface((2, H, 2 * W)), _iface((2, 9, 8)),       # a last axis that is not 2
                _iface((H, W, 2), (4 * W, 4, 2)),              # a sample stride that is not 1
                _iface((H, W, 2), (4 * W, 4, 1)),              # a pixel stride that is not 2
                _iface((H, W, 2), (2 * W - 1, 2, 1)),          # a pitch below 2 W
                _iface((H, W, 2), (1 << 23, 2, 1))):
        with pytest.raises(ValueError):
            DeviceFrames.from_cuda_array(bad, layout)
    with pytest.raises(ValueError):
        DeviceFrames.from_planes([(BASE,)], (W, H), layout, pitch=2 * W - 1)
    with pytest.raises(ValueError):
        DeviceFrames.from_planes([(BASE,)], (W - 1, H), layout, pitch=2 * W)
    with pytest.raises(ValueError):
        DeviceFrames.from_planes([(0,)], (W, H), layout, pitch=2 * W)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_host_frames_pack_into_one_pitched_plane(layout):
    H, W = 5, 6
    frames = np.random.default_rng(3).integers(0, 256, (2, H, W, 2), dtype=np.uint8)
    pitch, off = 2 * W + 5, 3
    block, surf, size, single = pack_host_frames(frames, layout, pitch=pitch, offset=off, fill=0xEE)
    assert size == (W, H) and not single and block.size == off + 2 * H * pitch - 5               # it ends on the last byte of the last row
    for k in range(2):
        at = int(surf["plane"][k, 0])
        rows = np.lib.stride_tricks.as_strided(block[at:], shape=(H, 2 * W), strides=(pitch, 1))
        assert np.array_equal(rows, frames[k].reshape(H, 2 * W))
    assert (np.delete(block, [int(surf["plane"][k, 0]) + r * pitch + c for k in range(2) for r in range(H) for c in range(2 * W)]) == 0xEE).all()
    assert pack_host_frames(frames[0], layout)[3]
    for bad in (np.zeros((H, W, 3), np.uint8), np.zeros((H, 2 * W), np.uint8), np.zeros((H, W + 1, 2), np.uint8)):
        with pytest.raises(ValueError):
            pack_host_frames(bad, layout)


class _Ctx(FakeContext):
    """The CPU stand-in with the calls a window makes before its first frame is touched: none of them may be reached."""

    def attach_device_frames(self, frames, first=0):
        raise AssertionError("a frame was touched")

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        raise AssertionError("a frame was touched")
    upload_frame_rows_async = upload_frames = upload_frame_rows

    def set_input_format(self, pixel_format, matrix="bt601"):
        self.layout = pixel_format


@pytest.mark.parametrize("layout", LAYOUTS)
def test_422_is_refused_as_a_destination_before_any_device_call(monkeypatch, layout):
    from lane_tracker_amd import calib
    from lane_tracker_amd.group import LaneTrackerGroup
    from lane_tracker_amd.lane_tracker import LaneTracker
    monkeypatch.setattr(_native, "Context", _Ctx)
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    rgb, t = LaneTracker(**cal), LaneTracker(**cal, pixel_format=layout, yuv_matrix="bt709")
    try:
        assert t._ctx.layout == layout and t._frame_shape == (H, W, 2)
        host = np.zeros((2, H, W, 2), np.uint8)
        feed = DeviceFrames.from_planes([(BASE,), (BASE + 2 * H * W,)], (W, H), layout, pitch=2 * W)
        sink422 = DeviceFrames.from_planes([(BASE,), (BASE + 2 * H * W,)], (W, H), layout, pitch=2 * W)
        rgb_host = np.zeros((2, H, W, 3), np.uint8)
        # a 4:2:2 container as out=, whatever the tracker's own format
        for tracker, frames in ((t, host), (t, feed), (rgb, rgb_host)):
            with pytest.raises(ValueError, match="input format only"):
                tracker.process_batch(frames, out=sink422)
            with pytest.raises(ValueError, match="input format only"):
                list(tracker.process_stream([frames], out=[sink422]))
        # nothing is drawn into 4:2:2 frames: out="inplace" and annotate="inplace"
        for frames in (feed, host):
            with pytest.raises(ValueError):
                t.process_batch(frames, out="inplace")
            with pytest.raises(ValueError):
                list(t.process_stream([frames], out="inplace"))
            with pytest.raises(ValueError):
                t.process_batch(frames, annotate="inplace")
            with pytest.raises(ValueError):
                list(t.process_stream([frames], annotate="inplace"))
        with pytest.raises(ValueError, match="input format only"):
            t.process_batch(feed, out="inplace", out_yuv_matrix="bt601")
        # frames of another shape or format
        for bad in (rgb_host, np.zeros((2, H * 3 // 2, W), np.uint8), np.zeros((2, H, 2 * W), np.uint8), np.zeros((H, W, 2), np.uint8)):
            with pytest.raises(ValueError):
                t.process_batch(bad, annotate=False)
        for bad in (np.zeros((H, W, 3), np.uint8), np.zeros((1, H, W, 2), np.uint8), np.zeros((H, 2 * W), np.uint8), None,
                    DeviceFrames.from_planes((BASE,), (W, H), "rgb", pitch=3 * W)):
            with pytest.raises(ValueError):
                t.process(bad)
        assert t.counter == 0 and rgb.counter == 0
        # the format's name travels in the state
        st = t.get_state()
        assert (st["pixel_format"], st["yuv_matrix"]) == (layout, "bt709")
        with pytest.raises(ValueError):
            rgb.set_state(st)
        twin = LaneTracker(**cal, pixel_format=layout, yuv_matrix="bt709")
        twin.set_state(st)
        twin.close()
    finally:
        rgb.close()
        t.close()
    with pytest.raises(ValueError):
        LaneTracker(**dict(cal, img_size=(W + 1, H)), pixel_format=layout)           # odd width
    odd = LaneTracker(**dict(cal, img_size=(W, H + 1)), pixel_format=layout)          # any height
    odd.close()
    g = LaneTrackerGroup(2, **cal, pixel_format=layout)
    try:
        assert g._ctx.layout == layout and all(m.pixel_format == layout for m in g.trackers)
        with pytest.raises(ValueError):
            g.process([np.zeros((H, W, 3), np.uint8), None], annotate=False)
    finally:
        g.close()
    with pytest.raises(ValueError, match="input format only"):
        from lane_tracker_amd import utils
        utils.rgb_to_yuv(np.zeros((4, 8, 3), np.uint8), layout)


# ---- raw 4:2:2 files ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_raw_422_files_round_trip_through_source_and_sink(tmp_path, layout):
    w, h = 18, 5
    frames = np.random.default_rng(1).integers(0, 256, (5, h, w, 2), dtype=np.uint8)
    path = str(tmp_path / ("clip." + layout))
    with video.FrameSink(path, (w, h), pixel_format=layout) as sink:
        sink.write(frames[:3])
        sink.write(frames[3])
        sink.write(frames[4:])
        with pytest.raises(ValueError):
            sink.write(np.zeros((h, w, 3), np.uint8))
    assert os.path.getsize(path) == 5 * h * w * 2
    with pytest.raises(ValueError):
        video.FrameSource(path)                                      # size is required, as for .rgb
    with pytest.raises(ValueError):
        video.FrameSource(path, size=(w, h + 1))                     # not a whole number of frames
    with pytest.raises(ValueError):
        video.FrameSource(path, size=(w // 2, 2 * h))                # an odd width
    src = video.FrameSource(path, size=(w, h))
    assert (src.pixel_format, len(src), src.size) == (layout, 5, (w, h))
    assert np.array_equal(src.read(1, 4), frames[1:4]) and src.read(1, 4).flags["C_CONTIGUOUS"]
    assert np.array_equal(np.stack(list(src)), frames)
    assert video.VideoFileClip(path, size=(w, h)).pixel_format == layout
    with pytest.raises(ValueError):
        video.FrameSink(str(tmp_path / "out.rgb"), (w, h), pixel_format=layout)
    with pytest.raises(ValueError):
        video.FrameSink(str(tmp_path / "out.nv12"), (w, h), pixel_format=layout)


# ---- header and binding ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_layouts_and_the_abi_stays():
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    for name, value in (("LT_INPUT_RGB", 0), ("LT_INPUT_NV12", 1), ("LT_INPUT_I420", 2), ("LT_INPUT_YUY2", 3), ("LT_INPUT_UYVY", 4)):
        assert re.search(r"\b%s = %d\b" % (name, value), header)
    assert _native.INPUT_FORMATS == {"rgb": 0, "nv12": 1, "i420": 2, "yuy2": 3, "uyvy": 4}
    assert _native.PACKED_422 == ("yuy2", "uyvy")
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    declared = set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native._SIGNATURES)                      # additive: no new lt_* name
