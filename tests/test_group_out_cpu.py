"""LaneTrackerGroup.process(out=...): what is refused, and that it is refused before a frame is touched -- on the CPU stand-in for the
device context, whose frame-touching calls fail the test when they are reached."""
import numpy as np
import pytest

from fake_context import FakeContext
from lane_tracker_amd import _native, calib
from lane_tracker_amd.device import DeviceFrames

BASE = 0x7f0000001000          # a made-up device address: nothing here dereferences it


class _Ctx(FakeContext):
    """The calls a tick makes before and when its first frame is touched: none of the latter may be reached."""

    def _touched(self, *args, **kwargs):
        raise AssertionError("a frame was touched")
    attach_device_frames = upload_frame_rows = upload_frame_rows_async = upload_frames = upload_frame_rows_list = _touched
    upload_frame_rest_list = device_frames_rest = mask_run = set_slot_calibrations = _touched
    overlay_run_to_surfaces_packed = overlay_run_inplace_packed = overlay_run_packed = store_wait = _touched

    def set_input_format(self, pixel_format, matrix="bt601"):
        self.layout = pixel_format


def _frames(k, size, pixel_format, readonly=False, n=1):
    """k one-frame DeviceFrames (n = 1) or one DeviceFrames of k surfaces (n = k) at made-up addresses."""
    w, h = size
    planes = {"rgb": lambda b: (b,), "nv12": lambda b: (b, b + w * h), "i420": lambda b: (b, b + w * h, b + w * h * 5 // 4),
              "yuy2": lambda b: (b,), "uyvy": lambda b: (b,)}[pixel_format]
    pitch = {"rgb": 3 * w, "yuy2": 2 * w, "uyvy": 2 * w}.get(pixel_format, w)
    cp = {"nv12": w, "i420": w // 2}.get(pixel_format)
    each = [DeviceFrames.from_planes(planes(BASE + i * 4 * w * h), size, pixel_format, pitch=pitch, chroma_pitch=cp) for i in range(k)]
    for f in each:
        f.readonly = readonly
    if n == 1:
        return each
    return DeviceFrames(np.concatenate([f.surfaces for f in each]), size, pixel_format)


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", _Ctx)


def _refusals(g, frames, cases):
    for what, kw in cases:
        with pytest.raises(ValueError):
            g.process(frames, **kw)
            pytest.fail("accepted: " + what)
    assert all(t.counter == 0 for t in g.trackers)


def test_refusals_of_an_rgb_group_come_before_any_device_call(fake):
    from lane_tracker_amd.group import LaneTrackerGroup
    cal = calib.reference_calibration()
    size = W, H = cal["img_size"]
    k = 3
    g = LaneTrackerGroup(k, **cal)
    try:
        host = [np.zeros((H, W, 3), np.uint8), None, np.zeros((H, W, 3), np.uint8)]
        dev = _frames(k, size, "rgb")
        sink = _frames(k, size, "nv12", n=k)
        elsewhere = _frames(k, size, "rgb", n=k)
        elsewhere.device = 1
        for frames in (host, dev):
            _refusals(g, frames, [
                ("out with annotate=False", dict(out=sink, annotate=False)),
                ("out with annotate='inplace'", dict(out=sink, annotate="inplace")),
                ("in place with annotate=False", dict(out="inplace", annotate=False)),
                ("a sink of two surfaces", dict(out=sink[0:2])),
                ("a sink of four surfaces", dict(out=_frames(k + 1, size, "rgb", n=k + 1))),
                ("a sink of another size", dict(out=_frames(k, (W, H - 2), "i420", n=k))),
                ("a sink on another device", dict(out=elsewhere)),
                ("a host array as the sink", dict(out=np.zeros((k, H, W, 3), np.uint8))),
                ("a list as the sink", dict(out=list(sink))),
                ("another string", dict(out="in-place")),
                ("an unknown matrix", dict(out=sink, out_yuv_matrix="bt2020")),
                ("seven coefficients", dict(out=sink, out_yuv_matrix=[1] * 7)),
            ])
            for fmt in ("yuy2", "uyvy"):
                with pytest.raises(ValueError, match="input format only"):
                    g.process(frames, out=_frames(k, size, fmt, n=k))
        # in place: host arrays and read-only frames have nowhere to draw
        _refusals(g, host, [("in place with host arrays", dict(out="inplace"))])
        mixed = [dev[0], None, host[2]]
        _refusals(g, mixed, [("in place with one host array", dict(out="inplace"))])
        frozen = _frames(k, size, "rgb", readonly=True)
        _refusals(g, [dev[0], frozen[1], None], [("in place with a read-only frame", dict(out="inplace"))])
        # what a group never offered stays what it was
        for kw in (dict(visualize_search=True), dict(split_view=True), dict(visualize_search=True, out=sink)):
            with pytest.raises(NotImplementedError):
                g.process(host, **kw)
        with pytest.raises(TypeError):
            g.process(host, out=sink, no_such_keyword=1)
        assert all(t.counter == 0 for t in g.trackers)
        # a tick in which every stream skips returns before the device as well, whatever the destination
        assert g.process([None] * k, out=sink) == [None] * k and g.process([None] * k, out="inplace") == [None] * k
    finally:
        g.close()


def test_refusals_of_yuv_groups(fake):
    from lane_tracker_amd.group import LaneTrackerGroup
    cal = calib.reference_calibration()
    size = W, H = cal["img_size"]
    k = 2
    custom = (1220542, 1673527, -852492, -409993, 2116027)
    g = LaneTrackerGroup(k, **cal, pixel_format="nv12", yuv_matrix=custom)
    try:
        dev = _frames(k, size, "nv12")
        # a custom input matrix names no matrix for the way back
        _refusals(g, dev, [("in place without out_yuv_matrix", dict(out="inplace")),
                           ("in place with an unknown matrix", dict(out="inplace", out_yuv_matrix="bt2020"))])
    finally:
        g.close()
    for fmt in ("yuy2", "uyvy"):
        g = LaneTrackerGroup(k, **cal, pixel_format=fmt)
        try:
            dev = _frames(k, size, fmt)
            for kw in (dict(out="inplace"), dict(out="inplace", out_yuv_matrix="bt601")):
                with pytest.raises(ValueError, match="input format only"):
                    g.process(dev, **kw)
            with pytest.raises(ValueError, match="input format only"):
                g.process(dev, out=_frames(k, size, fmt, n=k))
            assert all(t.counter == 0 for t in g.trackers)
        finally:
            g.close()


def test_select_takes_a_list_of_indices():
    size = (8, 4)
    f = _frames(4, size, "nv12", n=4)
    s = f.select([3, 0])
    assert len(s) == 2 and not s.single and s.pixel_format == "nv12" and s.img_size == size
    assert s.surfaces.tobytes() == f.surfaces[[3, 0]].tobytes()
    assert len(f.select([])) == 0
    with pytest.raises(IndexError):
        f.select([4])
