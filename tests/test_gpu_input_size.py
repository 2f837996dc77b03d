"""Frames of another size than the calibration's (`input_size=`, lt_set_input_size) on the device: everything is bit for bit what a plain
context / tracker gives when fed `oracle.resize_linear(frame, img_size)` -- cv2.resize with the default INTER_LINEAR.  The resize
where it lies (identity camera, every row and column); the camera frame of a slot after every family of uploads; trackers and a
group through process(), process_batch, process_stream and device sinks; refusals that leave the context usable."""
import ctypes as C

import numpy as np
import pytest

from lane_tracker_amd import _native, calib, synth, utils
from lane_tracker_amd.device import DeviceFrames
from oracle import oracle as O
from test_gpu_process_tail import _full

pytestmark = pytest.mark.gpu

W, H = 1280, 720


def _noise(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _resized(frames, size):
    return np.stack([O.resize_linear(f, size) for f in frames], 0)


# ---- 1. the resize where it lies: an identity camera, whose bird's-eye view reads every row ----------------------------------------------
@pytest.mark.parametrize("size,src", [((64, 48), (128, 96)),       # exact 2:1
                                      ((64, 48), (96, 72)),        # 3:2
                                      ((64, 48), (97, 55)),        # odd source row bytes, a ratio that is no fraction of small numbers
                                      ((64, 48), (48, 36)),        # upscale: clamped edge taps at both ends
                                      ((66, 50), (130, 75)),       # destination rows not dword-aligned
                                      ((37, 21), (59, 33))])       # destination rows not dword-aligned, odd everything
def test_resize_where_it_lies(size, src):
    w, h = size
    mk = lambda: _native.Context((w, h), (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=4)
    frames = _noise(w * 131 + src[0], 3, src[1], src[0])          # uniform bytes
    want = _resized(frames, (w, h))
    a, b = mk(), mk()
    try:
        a.set_input_size(src)
        assert a.input_size() == src and b.input_size() == (w, h)
        i = a.info()
        r0, r1 = i.src_row0, i.src_row1
        assert r0 == 0 and r1 >= h - 1                     # the bird's-eye view of this camera reads every row
        s0, s1 = a.input_rows()
        y0, y1, _, _ = utils._resize_taps(src[1], h)
        c0, c1 = a.source_rows()
        assert (s0, s1) == (int(y0[c0]), int(y1[c1 - 1]) + 1) and b.input_rows() == b.source_rows()
        assert a.set_direct_upload(-1) == 0                # its rows go to staging
        a.upload_frame_rows(frames, first=1)
        a.mask_run(3, first=1)
        und = a.download_undistorted(3, first=1)
        assert np.array_equal(und, want[:, r0:r1]), np.argwhere(und != want[:, r0:r1])[:4]
        b.upload_frame_rows(want, first=1)
        b.mask_run(3, first=1)
        assert np.array_equal(b.download_undistorted(3, first=1), und)
        for p in (0, 1):
            assert np.array_equal(a.download_plane(p, 3, first=1), b.download_plane(p, 3, first=1)), p
    finally:
        a.close()
        b.close()


# ---- 2. the camera frame of a slot ---------------------------------------------------------------------------------------------------------
def _read_back(c, n, first=0):
    """Every row of the camera frames of slots [first, first + n), whatever calls brought them, through the overlay with no points
    (a plain copy) over two runs of rows that cover the frame (a whole-frame overlay is refused while a slot holds row runs only)."""
    e = np.zeros(0, np.int64)
    rows = np.array([0, H // 2, H // 2, H], np.int32)
    c.overlay_run([(e, e, e, e)] * n, first=first, rows=rows.ctypes.data)
    out = _native.pinned_empty((n, H, W, 3))
    out[:] = 0
    c.download_overlay_async(out, first=first, rows=rows.ctypes.data)
    c.sync()
    return np.array(out)


def _mask_batch(c, frames):
    """lt_mask_batch: frames in, masks out, through slots 0 .."""
    f = np.ascontiguousarray(frames, np.uint8)
    out = np.empty((len(f), c.warp_h, c.warp_w), np.uint8)
    fp = _native.filter_params()
    _native._check(c.lib.lt_mask_batch(c._h, f.ctypes.data, len(f), C.byref(fp), out.ctypes.data))
    return out


@pytest.fixture(scope="module")
def camera_1080():
    """Eight scenes scaled up to 1920x1080 -- what a 1080p camera would deliver -- and their cv2.resize back to 1280x720, which is what
    a tracker with input_size=(1920, 1080) has to see.  No round-tripped frame equals its original scene."""
    r = synth.SceneRenderer()
    scenes = [r.render(i)[0] for i in range(8)]
    cam = np.stack([O.resize_linear(s, (1920, 1080)) for s in scenes], 0)
    back = _resized(cam, (W, H))
    assert not any(np.array_equal(b, s) for b, s in zip(back, scenes))
    return cam, back


def test_camera_frame_holds_the_resized_rows(camera_1080):
    cal = calib.reference_calibration()
    frames = np.concatenate([_noise(21, 2, 1080, 1920), camera_1080[0][3:4]])
    want = np.concatenate([_resized(frames[:2], (W, H)), camera_1080[1][3:4]])
    n = len(frames)
    c = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], capacity=4)
    try:
        c.set_input_size((1920, 1080))
        c.overlay_configure(cal["warp_matrices"][1])
        r0, r1 = c.source_rows()
        assert (r0, r1) != (0, H) and c.input_rows()[0] > 0 and c.input_rows()[1] < 1080
        c.upload_frames(frames, first=1)                                             # the whole frame
        assert np.array_equal(_read_back(c, n, first=1), want), "lt_upload_frames"
        other, exp = np.roll(frames, 1, 0), np.roll(want, 1, 0)                       # rows + rest: the whole frame from two calls
        keep = [c.upload_frame_rows(other, first=1, enqueue=True)]
        c.mask_run(n, first=1)
        keep.append(c.upload_frame_rest(other, first=1))
        got = _read_back(c, n, first=1)
        assert np.array_equal(got, exp), ("rows + rest", np.argwhere(got != exp)[:4])
        c.sync()
        # rows + rest_rows with two runs (odd bounds): the rows the path reads and those runs hold the new frame, every other row what
        # it held (`exp`)
        third, exp3 = np.roll(frames, 2, 0), np.roll(want, 2, 0)
        runs = (5, 62, r0 + 9, H - 3)
        rows = np.array(runs, np.int32)
        keep = [c.upload_frame_rows_async(np.ascontiguousarray(third), first=1)]
        c.mask_run(n, first=1)
        keep.append(c.upload_frame_rest(third, first=1, rows=rows.ctypes.data))
        got = _read_back(c, n, first=1)
        held = exp.copy()
        for lo, hi in ((runs[0], runs[1]), (runs[2], runs[3]), (r0, r1)):
            held[:, lo:hi] = exp3[:, lo:hi]
        assert np.array_equal(got, held), ("rows + rest_rows", np.argwhere(got != held)[:4])
        c.sync()
        # frames from separate arrays: the list forms, into other slots in another order
        sep = [np.array(frames[k]) for k in (2, 0, 1)]
        keep = [c.upload_frame_rows_list(sep, first=0)]
        c.mask_run(3, first=0)
        keep.append(c.upload_frame_rest_list(sep, first=0))
        got = _read_back(c, 3, first=0)
        assert np.array_equal(got, want[[2, 0, 1]]), ("rows_list + rest_list", np.argwhere(got != want[[2, 0, 1]])[:4])
        c.sync()
        # the synchronous rows upload, and the masks against a plain context fed the resized frames
        c.upload_frame_rows(frames, first=1)
        c.mask_run(n, first=1)
        p = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], capacity=4)
        try:
            p.overlay_configure(cal["warp_matrices"][1])
            p.upload_frame_rows(want, first=1)
            p.mask_run(n, first=1)
            assert np.array_equal(c.download_masks(n, first=1), p.download_masks(n, first=1))
            assert np.array_equal(_mask_batch(c, frames), _mask_batch(p, want))
        finally:
            p.close()
    finally:
        c.close()


# ---- 3. trackers -------------------------------------------------------------------------------------------------------------------------------
def _pair(cal, size):
    from lane_tracker_amd.lane_tracker import LaneTracker
    return LaneTracker(**cal, input_size=size), LaneTracker(**cal)


def _same(sized, plain, where):
    assert sized.get_state() == plain.get_state(), where
    assert _full(sized) == _full(plain), where
    assert sized.get_success_ratio() == plain.get_success_ratio(), where


def test_process_frame_by_frame(camera_1080):
    cam, back = camera_1080
    sized, plain = _pair(calib.reference_calibration(), (1920, 1080))
    try:
        assert sized.input_size == (1920, 1080) and plain.input_size is None
        for k in range(8):
            got, want = sized.process(cam[k]), plain.process(back[k])
            assert got.shape == (H, W, 3) and np.array_equal(got, want), (k, np.argwhere(got != want)[:4])
            _same(sized, plain, k)
            assert sized.valid_lane_lines, k
        assert sized.get_success_ratio() == (1.0, 8, 8)
        assert "input_size" not in sized.get_state()
        plain.set_state(sized.get_state())                 # a plain tracker's dict, either way
        sized.set_state(plain.get_state())
    finally:
        sized.close()
        plain.close()


def test_process_batch_and_a_nv12_sink(camera_1080):
    cam, back = camera_1080
    sized, plain = _pair(calib.reference_calibration(), (1920, 1080))
    sinks = [DeviceFrames.empty(4, (W, H), "nv12") for _ in range(2)]
    try:
        got, want = sized.process_batch(cam[:4]), plain.process_batch(back[:4])
        assert len(got) == 4 and all(np.array_equal(g, w) for g, w in zip(got, want))
        _same(sized, plain, "batch")
        sized.process_batch(cam[4:], out=sinks[0], out_yuv_matrix="bt709")
        plain.process_batch(back[4:], out=sinks[1], out_yuv_matrix="bt709")
        assert np.array_equal(sinks[0].to_host(), sinks[1].to_host())
        _same(sized, plain, "sink")
        assert sized.get_success_ratio() == (1.0, 8, 8)
        with pytest.raises(ValueError):                    # a sink of the input's size is not the tracker's
            sized.process_batch(cam[:4], out=DeviceFrames.from_planes([(sinks[0].owner.ptr,)] * 4, (1920, 1080), "rgb", pitch=3 * 1920))
    finally:
        sized.close()
        plain.close()
        for s in sinks:
            s.owner.close()


@pytest.mark.parametrize("annotate", [False, True], ids=["plain", "annotated"])
def test_process_stream_two_windows_of_four(camera_1080, annotate):
    cam, back = camera_1080
    sized, plain = _pair(calib.reference_calibration(), (1920, 1080))
    try:
        got = list(sized.process_stream([cam[:4], cam[4:]], annotate=annotate))
        want = list(plain.process_stream([back[:4], back[4:]], annotate=annotate))
        assert [len(w) for w in got] == [4, 4]
        for gw, ww in zip(got, want):
            for g, w in zip(gw, ww):
                assert (g is None and w is None) if not annotate else np.array_equal(g, w)
        _same(sized, plain, "stream")
        assert sized.get_success_ratio() == (1.0, 8, 8)
    finally:
        sized.close()
        plain.close()


def test_group_of_three_at_1600x900_equals_three_solo_plain_trackers():
    from lane_tracker_amd import LaneTrackerGroup
    from lane_tracker_amd.lane_tracker import LaneTracker
    cal = calib.reference_calibration()
    r = synth.SceneRenderer()
    cam = [[O.resize_linear(r.render(10 * i + t)[0], (1600, 900)) for t in range(3)] for i in range(3)]
    g = LaneTrackerGroup(3, **cal, input_size=(1600, 900))
    solos = [LaneTracker(**cal) for _ in range(3)]
    try:
        assert g.input_size == (1600, 900)
        for t in range(3):
            tick = [cam[i][t] if (i, t) != (1, 1) else None for i in range(3)]      # stream 1 skips a call
            outs = g.process(tick)
            for i, f in enumerate(tick):
                if f is None:
                    assert outs[i] is None
                    continue
                want = solos[i].process(O.resize_linear(f, (W, H)))
                assert outs[i].shape == (H, W, 3) and np.array_equal(outs[i], want), (t, i)
                _same(g.trackers[i], solos[i], (t, i))
        sink = DeviceFrames.empty(3, (W, H), "rgb")
        try:
            tick = [cam[i][0] for i in range(3)]
            g.process(tick, out=sink)
            for i in range(3):
                assert np.array_equal(sink.to_host()[i], solos[i].process(O.resize_linear(tick[i], (W, H)))), i
        finally:
            sink.owner.close()
    finally:
        g.close()
        for s in solos:
            s.close()


# ---- 4. refusals leave the context usable ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    w, h, src = 64, 48, (96, 72)
    mk = lambda: _native.Context((w, h), (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=2)
    frames = _noise(3, 2, src[1], src[0])
    want = _resized(frames, (w, h))

    def good(c, f, expect):
        c.upload_frame_rows(f)
        c.mask_run(2)
        r0, r1 = c.info().src_row0, c.info().src_row1
        assert np.array_equal(c.download_undistorted(2), expect[:, r0:r1])
    a = mk()
    try:                                                   # after an upload: LT_ERR_STATE, and the plain context goes on
        for bad in ((0, 5), (5, 0), (16385, 5), (5, 16385)):
            with pytest.raises(ValueError, match="16384"):     # LT_ERR_INVALID
                a.set_input_size(bad)
        good(a, want, want)
        with pytest.raises(_native.NativeError, match="after its first upload"):
            a.set_input_size(src)
        assert a.input_size() == (w, h)
        a.set_input_size((w, h))                           # no change: fine
        good(a, want[::-1], want[::-1])
    finally:
        a.close()
    a = mk()
    try:                                                   # on an NV12 context; and a YUV layout on a context with an input size
        a.set_input_format("nv12")
        with pytest.raises(_native.NativeError, match="RGB"):
            a.set_input_size(src)
        assert a.input_size() == (w, h) and a.input_format()[0] == "nv12"
    finally:
        a.close()
    a = mk()
    dev = DeviceFrames.empty(2, (w, h), "rgb")
    try:
        a.set_input_size(src)
        with pytest.raises(ValueError):
            a.set_input_format("nv12")
        k = np.array([1220542, 1673527, -852492, -409993, 2116026], np.int32)
        assert a.lib.lt_set_input_format(a._h, 1, k.ctypes.data) == -5 and b"input size" in a.lib.lt_last_error()      # LT_ERR_STATE
        assert a.input_format()[0] == "rgb"
        # frames in device memory: refused by the binding, and by the library itself with nothing launched
        with pytest.raises(ValueError, match="device memory"):
            a.attach_device_frames(dev)
        s = np.ascontiguousarray(dev.surfaces)
        assert a.lib.lt_attach_device_frames(a._h, s.ctypes.data, 0, 2) == -5 and b"device memory" in a.lib.lt_last_error()
        # frames of the wrong shape: the calibration's own size, a transposed frame, a whole number of other frames
        for bad in (want, frames.transpose(0, 2, 1, 3), np.zeros((3, src[1] * src[0] * 2), np.uint8)):
            with pytest.raises(ValueError):
                a.upload_frame_rows(bad)
            with pytest.raises(ValueError):
                a.upload_frames(bad)
        good(a, frames, want)
        a.set_input_size(src)                              # the same size again: fine after an upload
        with pytest.raises(_native.NativeError, match="after its first upload"):
            a.set_input_size((w, h))
        good(a, frames[::-1], want[::-1])
    finally:
        a.close()
        dev.owner.close()
