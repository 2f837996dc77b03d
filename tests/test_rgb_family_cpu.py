"""BGR / RGBA / BGRA input and sinks without a GPU: the format tables and the two NumPy functions of `utils` (the definition: a
channel permutation, alpha dropped); what `DeviceFrames` packs, parses and refuses; raw `.bgr` / `.rgba` / `.bgra` files; what a
tracker and a group refuse before any device call; the C header."""
import os
import re

import numpy as np
import pytest

from fake_context import FakeContext
from lane_tracker_amd import _native, utils, video
from lane_tracker_amd.device import DeviceFrames, pack_host_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ["bgr", "rgba", "bgra"]
BPP = {"bgr": 3, "rgba": 4, "bgra": 4}
BASE = 0x7f0000001000          # a made-up device address: nothing here dereferences it


def to_rgb(f, fmt):
    """The issue's definition, written out."""
    return {"bgr": lambda a: a[..., ::-1], "rgba": lambda a: a[..., :3], "bgra": lambda a: a[..., 2::-1]}[fmt](f)


# ---- tables and the NumPy functions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_shape_and_format_tables(fmt):
    assert _native.frame_shape((64, 48), fmt) == (48, 64, BPP[fmt])
    assert _native.frame_shape((3, 1), fmt) == (1, 3, BPP[fmt])               # no parity requirement
    assert _native.frame_shape((2, 7), fmt) == (7, 2, BPP[fmt])               # the narrowest frame
    assert _native.frame_shape((1, 1), fmt) == (1, 1, BPP[fmt])               # (a sink may be one pixel wide ...
    with pytest.raises(ValueError):
        _native.input_frame_shape((1, 48), fmt)                               # ... a camera frame not)
    assert _native.input_frame_shape((2, 7), fmt) == (7, 2, BPP[fmt])
    for size in ((0, 48), (8, 0)):
        with pytest.raises(ValueError):
            _native.frame_shape(size, fmt)
    want = {"bgr": 5, "rgba": 6, "bgra": 7}[fmt]
    assert _native.pixel_format_id(fmt) == want == _native.RGB_FAMILY[fmt] == _native.sink_format_id(fmt)
    assert _native.format_name(want) == fmt and not _native.is_yuv(want)
    with pytest.raises(ValueError):
        _native.draw_sink_format_id(fmt)                                      # (the one-launch draw of a group)
    assert [_native.draw_sink_format_id(f) for f in ("rgb", "nv12", "i420")] == [0, 1, 2]
    with pytest.raises(ValueError):
        _native.checked_input_size((32, 24), (64, 48), fmt)
    assert _native.checked_input_size((64, 48), (64, 48), fmt) is None       # the calibration's own size is no input size


def test_the_pinned_tables_keep_their_contents():
    assert _native.PIXEL_FORMATS == {"rgb": 0, "nv12": 1, "i420": 2}
    assert _native.INPUT_FORMATS == {"rgb": 0, "nv12": 1, "i420": 2, "yuy2": 3, "uyvy": 4}
    assert _native.PACKED_422 == ("yuy2", "uyvy")
    assert _native.RGB_FAMILY == {"bgr": 5, "rgba": 6, "bgra": 7}
    with pytest.raises(ValueError):
        _native.pixel_format_id("argb")
    with pytest.raises(ValueError):
        _native.pixel_format_id(None)


@pytest.mark.parametrize("fmt", FORMATS)
def test_packed_to_rgb_and_back(fmt):
    rng = np.random.default_rng(7)
    f = rng.integers(0, 256, (3, 5, 7, BPP[fmt]), dtype=np.uint8)            # random alpha
    rgb = utils.packed_to_rgb(f, fmt)
    assert rgb.shape == (3, 5, 7, 3) and rgb.flags["C_CONTIGUOUS"] and np.array_equal(rgb, to_rgb(f, fmt))
    assert np.array_equal(utils.packed_to_rgb(f[0], fmt), to_rgb(f[0], fmt))
    back = utils.rgb_to_packed(rgb, fmt)
    assert back.shape == f.shape and np.array_equal(utils.packed_to_rgb(back, fmt), rgb)       # the round trip
    if BPP[fmt] == 4:
        assert (back[..., 3] == 255).all() and np.array_equal(back[..., :3], f[..., :3])       # alpha dropped, written as 255
        assert (utils.rgb_to_packed(rgb, fmt, alpha=7)[..., 3] == 7).all()
    else:
        assert np.array_equal(back, f)
    # a single pixel written out
    px = np.array([[[10, 20, 30]]], np.uint8)
    assert utils.rgb_to_packed(px, fmt).reshape(-1).tolist() == {"bgr": [30, 20, 10], "rgba": [10, 20, 30, 255], "bgra": [30, 20, 10, 255]}[fmt]
    assert np.array_equal(utils.packed_to_rgb(px, "rgb"), px) and np.array_equal(utils.rgb_to_packed(px, "rgb"), px)
    for bad in (np.zeros((5, 7, 7 - BPP[fmt]), np.uint8), np.zeros((5, 7), np.uint8), np.zeros((5, 7, BPP[fmt]), np.float32)):
        with pytest.raises(ValueError):
            utils.packed_to_rgb(bad, fmt)
    with pytest.raises(ValueError):
        utils.rgb_to_packed(np.zeros((5, 7, 4), np.uint8), fmt)
    with pytest.raises(ValueError):
        utils.packed_to_rgb(f, "nv12")


# ---- DeviceFrames ---------------------------------------------------------------------------------------------------------------
def _iface(shape, strides=None, ptr=BASE, **more):
    return dict({"shape": tuple(shape), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": strides}, **more)


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_frames_from_cuda_array_and_planes(fmt):
    H, W, b = 5, 7, BPP[fmt]
    for pitch in (b * W, b * W + 5):
        one = DeviceFrames.from_cuda_array(_iface((H, W, b), (pitch, b, 1)), fmt)
        assert one.single and len(one) == 1 and one.img_size == (W, H) and one.shape == (H, W, b) and one.pixel_format == fmt
        assert int(one.surfaces["plane"][0, 0]) == BASE and int(one.surfaces["pitch"][0]) == pitch and not one.surfaces["plane"][0, 1:].any()
        fs = H * pitch + 11
        many = DeviceFrames.from_cuda_array(_iface((3, H, W, b), (fs, pitch, b, 1)), fmt)
        assert not many.single and many.shape == (3, H, W, b)
        assert [int(p) for p in many.surfaces["plane"][:, 0]] == [BASE + k * fs for k in range(3)] and set(many.surfaces["pitch"]) == {pitch}
        p = DeviceFrames.from_planes([(BASE,), (BASE + fs,)], (W, H), fmt, pitch=pitch)               # one plane, no chroma pitch
        assert len(p) == 2 and p.shape == (2, H, W, b) and set(p.surfaces["pitch"]) == {pitch} and set(p.surfaces["chroma_pitch"]) == {0}
        assert DeviceFrames.from_planes((BASE,), (W, H), fmt, pitch=pitch).single
    dense = DeviceFrames.from_cuda_array(_iface((2, H, W, b)), fmt)                                    # no strides: C order
    assert set(dense.surfaces["pitch"]) == {b * W} and int(dense.surfaces["plane"][1, 0]) == BASE + H * W * b
    other = 7 - b                                                                                      # the other family's last axis
    for bad in (_iface((H, W, other)),                         # (..., 3) given as 'rgba' / (..., 4) given as 'bgr'
                _iface((H, W, 2)), _iface((H, b * W)),
                _iface((H, W, b), (b * W - 1, b, 1)),          # a pitch below a row
                _iface((H, W, b), (2 * b * W, 2 * b, 1)),      # a pixel stride that is not the pixel's size
                _iface((H, W, b), (2 * b * W, b, 2)),          # a channel stride that is not 1
                _iface((H, W, b), (1 << 23, b, 1))):
        with pytest.raises(ValueError):
            DeviceFrames.from_cuda_array(bad, fmt)
    if b == 4:
        with pytest.raises(ValueError, match="pixel stride of 4"):
            DeviceFrames.from_cuda_array(_iface((H, W, 4), (8 * W, 8, 1)), fmt)
    with pytest.raises(ValueError):
        DeviceFrames.from_planes([(BASE,)], (W, H), fmt, pitch=b * W - 1)
    with pytest.raises(ValueError):
        DeviceFrames.from_planes([(0,)], (W, H), fmt, pitch=b * W)
    with pytest.raises(ValueError):
        DeviceFrames.from_planes([(BASE,)], (W, H), fmt, pitch=b * W).check_for((W, H), "rgb")
    with pytest.raises(ValueError):
        DeviceFrames.from_planes([(BASE,)], (W, H), "rgb", pitch=4 * W).check_for((W, H), fmt)
    DeviceFrames.from_planes([(BASE,)], (W, H), fmt, pitch=b * W).check_for((W, H), fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_frames_pack_into_one_pitched_plane(fmt):
    H, W, b = 5, 7, BPP[fmt]
    frames = np.random.default_rng(3).integers(0, 256, (2, H, W, b), dtype=np.uint8)
    pitch, off = b * W + 5, 3
    block, surf, size, single = pack_host_frames(frames, fmt, pitch=pitch, offset=off, fill=0xEE)
    assert size == (W, H) and not single and block.size == off + 2 * H * pitch - 5               # it ends on the last byte of the last row
    for k in range(2):
        at = int(surf["plane"][k, 0])
        rows = np.lib.stride_tricks.as_strided(block[at:], shape=(H, b * W), strides=(pitch, 1))
        assert np.array_equal(rows, frames[k].reshape(H, b * W))
    assert (np.delete(block, [int(surf["plane"][k, 0]) + r * pitch + c for k in range(2) for r in range(H) for c in range(b * W)]) == 0xEE).all()
    assert pack_host_frames(frames[0], fmt)[3]
    for bad in (np.zeros((H, W, 7 - b), np.uint8), np.zeros((H, b * W), np.uint8), np.zeros((H, W, 2), np.uint8)):
        with pytest.raises(ValueError):
            pack_host_frames(bad, fmt)
    with pytest.raises(ValueError):
        pack_host_frames(frames, fmt, pitch=b * W - 1)


# ---- raw files --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_raw_files_round_trip_through_source_and_sink(tmp_path, fmt):
    w, h, b = 7, 5, BPP[fmt]
    frames = np.random.default_rng(1).integers(0, 256, (5, h, w, b), dtype=np.uint8)
    path = str(tmp_path / ("clip." + fmt))
    with video.FrameSink(path, (w, h), pixel_format=fmt) as sink:
        sink.write(frames[:3])
        sink.write(frames[3])
        sink.write(frames[4:])
        with pytest.raises(ValueError):
            sink.write(np.zeros((h, w, 7 - b), np.uint8))
    assert os.path.getsize(path) == 5 * h * w * b
    with pytest.raises(ValueError):
        video.FrameSource(path)                                      # size is required, as for .rgb
    with pytest.raises(ValueError):
        video.FrameSource(path, size=(w, h + 1))                     # not a whole number of frames
    src = video.FrameSource(path, size=(w, h))
    assert (src.pixel_format, len(src), src.size) == (fmt, 5, (w, h))
    assert np.array_equal(src.read(1, 4), frames[1:4]) and src.read(1, 4).flags["C_CONTIGUOUS"]
    assert np.array_equal(np.stack(list(src)), frames)
    with pytest.raises(ValueError):
        video.FrameSink(str(tmp_path / "out.rgb"), (w, h), pixel_format=fmt)
    with pytest.raises(ValueError):
        video.FrameSink(str(tmp_path / ("out." + ("bgr" if fmt != "bgr" else "bgra"))), (w, h), pixel_format=fmt)


# ---- trackers: refusals before any device call --------------------------------------------------------------------------------
class _Ctx(FakeContext):
    """The CPU stand-in with the calls a window makes before its first frame is touched: none of them may be reached."""

    def attach_device_frames(self, frames, first=0):
        raise AssertionError("a frame was touched")

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        raise AssertionError("a frame was touched")
    upload_frame_rows_async = upload_frames = upload_frame_rows_list = upload_frame_rows

    def set_input_format(self, pixel_format, matrix="bt601"):
        self.layout = pixel_format


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_tracker_takes_the_format_and_refuses_before_any_device_call(monkeypatch, fmt):
    """Fails without the feature: LaneTracker(..., pixel_format='bgr') raises ValueError."""
    from lane_tracker_amd import calib
    from lane_tracker_amd.group import LaneTrackerGroup
    from lane_tracker_amd.lane_tracker import LaneTracker
    monkeypatch.setattr(_native, "Context", _Ctx)
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    b = BPP[fmt]
    rgb, t = LaneTracker(**cal), LaneTracker(**cal, pixel_format=fmt, yuv_matrix="no such matrix")     # (ignored, as for 'rgb')
    try:
        assert t._ctx.layout == fmt and t._frame_shape == (H, W, b)
        host = np.zeros((2, H, W, b), np.uint8)
        feed = DeviceFrames.from_planes([(BASE,), (BASE + b * H * W,)], (W, H), fmt, pitch=b * W)
        # nothing is drawn into such frames: out="inplace" and annotate="inplace"
        for frames in (feed, host):
            with pytest.raises(ValueError):
                t.process_batch(frames, out="inplace")
            with pytest.raises(ValueError):
                list(t.process_stream([frames], out="inplace"))
            with pytest.raises(ValueError):
                t.process_batch(frames, annotate="inplace")
            with pytest.raises(ValueError):
                list(t.process_stream([frames], annotate="inplace"))
        with pytest.raises(ValueError, match="out= sink"):
            t.process_batch(feed, out="inplace", out_yuv_matrix="bt601")
        # host frames never travel as row runs copied by the host: they are not RGB
        assert t._rows_for(np.zeros((H, W, 3), np.uint8)) is None and t._rows_for_window(np.zeros((2, H, W, 3), np.uint8)) is None
        # frames of another shape or format
        for bad in (np.zeros((2, H, W, 7 - b), np.uint8), np.zeros((2, H * 3 // 2, W), np.uint8), np.zeros((H, W, b), np.uint8)):
            with pytest.raises(ValueError):
                t.process_batch(bad, annotate=False)
        for bad in (np.zeros((H, W, 7 - b), np.uint8), np.zeros((1, H, W, b), np.uint8), None,
                    DeviceFrames.from_planes((BASE,), (W, H), "rgb", pitch=4 * W)):
            with pytest.raises(ValueError):
                t.process(bad)
        with pytest.raises(ValueError):
            rgb.process(DeviceFrames.from_planes((BASE,), (W, H), fmt, pitch=b * W))
        assert t.counter == 0 and rgb.counter == 0
        # the format's name travels in the state
        st = t.get_state()
        assert st["pixel_format"] == fmt
        with pytest.raises(ValueError):
            rgb.set_state(st)
    finally:
        rgb.close()
        t.close()
    with pytest.raises(ValueError):
        LaneTracker(**cal, pixel_format=fmt, input_size=(W // 2, H // 2))             # these frames are not resized
    with pytest.raises(ValueError):
        LaneTracker(**dict(cal, img_size=(1, H)), pixel_format=fmt)                   # width 1
    g = LaneTrackerGroup(2, **cal, pixel_format=fmt)
    try:
        assert g._ctx.layout == fmt and all(m.pixel_format == fmt for m in g.trackers)
        with pytest.raises(ValueError):
            g.process([np.zeros((H, W, 7 - b), np.uint8), None], annotate=False)
        with pytest.raises(ValueError):
            g.process([np.zeros((H, W, b), np.uint8), None], out="inplace")
    finally:
        g.close()
    with pytest.raises(ValueError):
        LaneTrackerGroup(2, **cal, pixel_format=fmt, input_size=(W // 2, H // 2))
    # a group's out= sink in one of these formats, whatever the group's own format
    sink = DeviceFrames.from_planes([(BASE,), (BASE + b * H * W,)], (W, H), fmt, pitch=b * W)
    g = LaneTrackerGroup(2, **cal)
    try:
        with pytest.raises(ValueError, match="group's out= sink"):
            g.process([np.zeros((H, W, 3), np.uint8)] * 2, out=sink)
    finally:
        g.close()
    with pytest.raises(ValueError):
        utils.rgb_to_yuv(np.zeros((4, 8, 3), np.uint8), fmt)
    with pytest.raises(ValueError):
        utils.yuv_to_rgb(np.zeros((4, 8, b), np.uint8), fmt)


# ---- header and binding ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_layouts_and_the_abi_stays():
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    for name, value in (("LT_INPUT_RGB", 0), ("LT_INPUT_NV12", 1), ("LT_INPUT_I420", 2), ("LT_INPUT_YUY2", 3), ("LT_INPUT_UYVY", 4),
                        ("LT_INPUT_BGR", 5), ("LT_INPUT_RGBA", 6), ("LT_INPUT_BGRA", 7)):
        assert re.search(r"\b%s = %d\b" % (name, value), header)
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    declared = set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native._SIGNATURES)                      # additive: no new lt_* name
