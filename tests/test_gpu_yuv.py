"""Camera frames in YUV 4:2:0 (NV12 / I420), converted on the device.  Everything here is bit for bit: the device conversion is
the integer formula `tests/yuv_reference.py` restates, and everything behind it is the existing path -- so a 4:2:0 context or
tracker must give exactly what an RGB one gives on the converted frames.  There is no tolerance anywhere."""
import numpy as np
import pytest

import yuv_reference as R
from lane_tracker_amd import _native, calib, synth

pytestmark = pytest.mark.gpu

LAYOUTS = ("nv12", "i420")
W, H = calib.IMAGE_WIDTH_HEIGHT


def _ctx(cal, capacity, pixel_format="rgb", matrix="bt601"):
    c = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                        capacity=capacity)
    if pixel_format != "rgb":
        c.set_input_format(pixel_format, matrix)
    return c


def _noise(seed, n=1, h=H, w=W):
    return np.random.default_rng(seed).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)


def _scenes(seeds, layout):
    r = synth.SceneRenderer()
    return np.stack([R.rgb_to_yuv420(r.render(int(s))[0], layout) for s in seeds])


def _to_rgb(frames, layout, matrix="bt601"):
    return np.stack([R.yuv420_to_rgb(f, layout, matrix) for f in frames])


def _valid_lanes(records):
    """How many of the records show both lines detected and a lane check_validity accepts (an RGB tracker's own check)."""
    from lane_tracker_amd.lane_tracker import LaneTracker
    cal = calib.reference_calibration()
    t = LaneTracker(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"], cal["mpp_conversion"])
    try:
        ok = 0
        for r in records:
            if r["detected"] and not r["fit_flags"]:
                t.check_validity(r["left_coeffs"], r["right_coeffs"])        # (sets valid_lane_lines, as the reference's does)
                ok += bool(t.valid_lane_lines)
        return ok
    finally:
        t.close()


# ---- the conversion itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1280, 720), (1920, 1080), (66, 34)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_yuv_to_rgb_is_the_restatement(layout, matrix, size):
    from lane_tracker_amd import utils
    w, h = size
    frame = _noise(h * 7 + w, 1, h, w)[0]          # uniform bytes: every clamp is hit
    got = utils.yuv_to_rgb(frame, layout=layout, matrix=matrix)
    want = R.yuv420_to_rgb(frame, layout, matrix)
    assert got.shape == (h, w, 3) and got.dtype == np.uint8
    assert (want == 0).any() and (want == 255).any()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_input_format_is_set_once_and_checked():
    cal = calib.reference_calibration()
    c = _ctx(cal, 2)
    try:
        assert c.input_format()[0] == "rgb"
        c.set_input_format("nv12", "bt709")
        assert c.input_format() == ("nv12", R.MATRICES["bt709"])
        c.set_input_format("i420", "bt601")                      # nothing uploaded yet: still free
        assert c.set_direct_upload(True) == 0                    # 4:2:0 rows take the engine
        with pytest.raises(ValueError):
            c.upload_frames(np.zeros((1, H, W, 3), np.uint8))    # an RGB frame into a 4:2:0 context
        c.upload_frames(_noise(1))
        c.set_input_format("i420", "bt601")                      # the same again is no change
        with pytest.raises(_native.NativeError):
            c.set_input_format("nv12", "bt601")
        with pytest.raises(_native.NativeError):
            c.set_input_format("rgb")
        with pytest.raises(ValueError):
            c.set_input_format("i420", (1 << 23, 0, 0, 0, 0))
    finally:
        c.close()
    odd = _native.Context((65, 34), (8, 8), np.eye(3), np.zeros(5), np.eye(3), capacity=1)
    try:
        with pytest.raises(ValueError):
            odd.set_input_format("nv12")
        assert odd.lib.lt_set_input_format(odd._h, 1, R_K601.ctypes.data) == -1      # LT_ERR_INVALID from the library itself
    finally:
        odd.close()


R_K601 = np.array(R.MATRICES["bt601"], np.int32)


# ---- the mask chain of a 4:2:0 context = that of an RGB context given the converted frames ---------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_mask_chain_parity_with_an_rgb_context(layout):
    cal = calib.reference_calibration()
    cap = 66
    scenes = _scenes(range(10), layout)
    frames = np.concatenate([scenes, _noise(11, 6), _scenes(range(10, 58), layout)])          # 64: scenes and uniform noise
    rgb = _to_rgb(frames, layout)
    a, b = _ctx(cal, cap, layout), _ctx(cal, cap)
    try:
        # the scenes must be ones a tracker FINDS lanes in, after the 4:2:0 round trip: asked of the RGB path before anything is compared
        b.upload_frame_rows(rgb[:10])
        b.mask_run(10)
        b.sws_fit_run(10)
        assert _valid_lanes(b.download_records(10)) >= 9
        for n, first in ((1, 0), (1, 1), (2, 0), (2, 3), (3, 0), (3, 1), (16, 0), (16, 5), (64, 0), (64, 1)):
            rot = (n + first) % 7                                                       # other frames in the slots every time
            fy, fr = np.roll(frames, rot, 0)[:n], np.roll(rgb, rot, 0)[:n]
            a.upload_frame_rows(fy, first=first)
            b.upload_frame_rows(fr, first=first)
            for c in (a, b):
                c.mask_run(n, first=first)
                c.sws_fit_run(n, first=first)
            what = "%s n=%d first=%d" % (layout, n, first)
            assert np.array_equal(a.download_undistorted(n, first=first), b.download_undistorted(n, first=first)), what
            for plane in range(6):
                assert np.array_equal(a.download_plane(plane, n, first=first), b.download_plane(plane, n, first=first)), (what, plane)
            assert np.array_equal(a.download_masks(n, first=first), b.download_masks(n, first=first)), what
            assert a.download_records(n, first=first).tobytes() == b.download_records(n, first=first).tobytes(), what
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_enqueued_and_stream_ordered_row_uploads_reuse_their_slots(layout):
    """The upload forms nobody waits for, over two slots that are written again while the device may still read them."""
    cal = calib.reference_calibration()
    frames = np.concatenate([_scenes(range(4), layout), _noise(3, 4)])[[0, 4, 1, 5, 2, 6, 3, 7]]
    rgb = _to_rgb(frames, layout)
    a, b = _ctx(cal, 2, layout), _ctx(cal, 2)
    keep = []
    try:
        for form in ("enqueue", "async", "list"):
            for k in range(len(frames)):
                slot = k & 1
                if form == "enqueue":
                    keep.append(a.upload_frame_rows(frames[k][None], first=slot, enqueue=True))
                elif form == "async":
                    keep.append(a.upload_frame_rows_async(np.ascontiguousarray(frames[k][None]), first=slot))
                else:
                    keep.append(a.upload_frame_rows_list([frames[k]], first=slot))
                b.upload_frame_rows(rgb[k][None], first=slot)
                for c in (a, b):
                    c.mask_run(1, first=slot)
                    c.sws_fit_run(1, first=slot)
                assert np.array_equal(a.download_masks(1, first=slot), b.download_masks(1, first=slot)), (form, k)
                assert a.download_records(1, first=slot).tobytes() == b.download_records(1, first=slot).tobytes(), (form, k)
    finally:
        a.close()
        b.close()


# ---- the RGB camera frame of a slot: whatever the RGB forms of a call sequence make valid holds the converted frame ---------------
def _read_back(c, n, first=0, rows=None):
    """The camera frames of slots [first, first + n) through the overlay with no points (a plain copy of the frame)."""
    e = np.zeros(0, np.int64)
    if rows is None:
        c.overlay_run([(e, e, e, e)] * n, first=first)
        return c.download_overlay(n, first=first)
    c.overlay_run([(e, e, e, e)] * n, first=first, rows=rows.ctypes.data)
    out = _native.pinned_empty((n, H, W, 3))
    out[:] = 0
    c.download_overlay_async(out, first=first, rows=rows.ctypes.data)
    c.sync()
    return np.array(out)


@pytest.mark.parametrize("configured_first", [True, False], ids=["rows_widened_first", "configured_after_upload"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_camera_frame_holds_the_converted_frame(layout, configured_first):
    cal = calib.reference_calibration()
    frames = np.concatenate([_noise(21, 3), _scenes([3], layout)])
    want = _to_rgb(frames, layout, "bt709")
    n = len(frames)
    c = _ctx(cal, 6, layout, "bt709")
    try:
        before = c.source_rows()
        if configured_first:
            c.overlay_configure(cal["warp_matrices"][1])
        print("source rows", before, "->", c.source_rows())
        # lt_upload_frames: the whole frame
        c.upload_frames(frames, first=1)
        if not configured_first:
            c.overlay_configure(cal["warp_matrices"][1])
        assert np.array_equal(_read_back(c, n, first=1), want), "lt_upload_frames"
        # rows + rest: the whole frame again, from two calls (and a mask run between them, as a stream does it)
        other = np.roll(frames, 1, 0)
        keep = [c.upload_frame_rows(other, first=2, enqueue=True)]
        c.mask_run(n, first=2)
        keep.append(c.upload_frame_rest(other, first=2))
        assert np.array_equal(_read_back(c, n, first=2), np.roll(want, 1, 0)), "rows + rest"
        c.sync()
        # rows + rest_rows with two runs (odd bounds among them): those runs, source rows included where a run covers them
        r0, r1 = c.source_rows()
        for runs in ((5, 62, r0 + 9, H - 3), (0, 1, r0 - 7, r1 + 1), (r0 + 1, r0 + 2, H - 1, H)):
            rows = np.array(runs, np.int32)
            third = np.roll(frames, 2 + runs[0] % 2, 0)
            keep = [c.upload_frame_rows(third, first=0, enqueue=True)]
            c.mask_run(n, first=0)
            keep.append(c.upload_frame_rest(third, first=0, rows=rows.ctypes.data))
            got = _read_back(c, n, first=0, rows=rows)
            exp = np.roll(want, 2 + runs[0] % 2, 0)
            for lo, hi in ((runs[0], runs[1]), (runs[2], runs[3])):
                assert np.array_equal(got[:, lo:hi], exp[:, lo:hi]), ("rows + rest_rows", runs, lo, hi)
            c.sync()
    finally:
        c.close()


# ---- trackers: a 4:2:0 tracker = an RGB tracker on the converted frames, annotated frames included -------------------------------
from lane_tracker_amd.lane_tracker import LaneTracker      # noqa: E402


def _state(lt):
    b = lambda a: None if a is None else np.asarray(a).tobytes()
    return dict(detected=lt.detected_pixels, valid=lt.valid_lane_lines, last_detection=lt.last_detection, success=lt.success,
                counter=lt.counter, left_avg=b(lt.left_avg_coeffs), right_avg=b(lt.right_avg_coeffs), last_left=b(lt.last_left_coeffs),
                last_right=b(lt.last_right_coeffs), hist=[b(c) for c in lt.left_fit_coeffs] + [b(c) for c in lt.right_fit_coeffs],
                radii=list(lt.average_curve_radii), radius=lt.average_curve_radius, ecc=lt.eccentricity,
                pix=(b(lt.left_y), b(lt.left_x), b(lt.right_y), b(lt.right_x)), cent=(lt.left_window_centroids, lt.right_window_centroids))


def _stream(n, layout, seed, blank=()):
    """A drifting lane as 4:2:0 frames (and the RGB frames they convert to); `blank`: positions of black frames."""
    rgb = synth.stream_lanes(n, seed=seed)
    yuv = np.stack([R.rgb_to_yuv420(f, layout) for f in rgb])
    black = np.concatenate([np.full((H, W), 16, np.uint8), np.full((H // 2, W), 128, np.uint8)])
    for k in blank:
        yuv[k] = black
    return yuv, _to_rgb(yuv, layout)


def _pair(layout, **kw):
    cal = calib.reference_calibration()
    return LaneTracker(**cal, pixel_format=layout, **kw), LaneTracker(**cal)


def _assert_lanes_found(rgb_tracker, seen):
    """The scenes must be ones the tracker finds lanes in: at least 9 of 10 non-blank frames valid on the RGB path."""
    assert rgb_tracker.success * 10 >= seen * 9, (rgb_tracker.success, seen)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_process_equals_an_rgb_tracker_on_the_converted_frames(layout):
    blank = tuple(range(14, 22))                       # an outage beyond n_reset: failure pictures, second tries, the sliding-window restart
    yuv, rgb = _stream(40, layout, 7, blank)
    a, b = _pair(layout)
    try:
        states = []
        for k in range(40):
            out_b = b.process(rgb[k])
            states.append(_state(b))
            out_a = a.process(yuv[k])
            assert out_a.shape == (H, W, 3) and np.array_equal(out_a, out_b), k
            assert _state(a) == states[-1], k
        _assert_lanes_found(b, 40 - len(blank))
        assert b.success < b.counter                   # ... and the failure path ran
        sa, sb = a.get_state(), b.get_state()
        assert sa.pop("pixel_format") == layout and sa.pop("yuv_matrix") == "bt601" and sa == sb
        # the pictures process() can return besides the annotated frame work from the converted frame
        va, vb = a.process(yuv[3], visualize_search=True), b.process(rgb[3], visualize_search=True)
        assert all(np.array_equal(x, y) for x, y in zip(va, vb))
        assert np.array_equal(a.process(yuv[4], split_view=True), b.process(rgb[4], split_view=True))
        with pytest.raises(ValueError):
            a.process(rgb[5])
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_process_batch_and_stream_equal_an_rgb_tracker(layout):
    yuv, rgb = _stream(48, layout, 11, blank=(20, 21, 22))
    for annotate in (False, True):
        a, b = _pair(layout)
        try:
            oa, ob = a.process_batch(yuv[:24], annotate=annotate), b.process_batch(rgb[:24], annotate=annotate)
            assert _state(a) == _state(b), annotate
            if annotate:
                assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
            else:
                assert oa == ob == [None] * 24
            _assert_lanes_found(b, 21)
            with pytest.raises(ValueError):
                a.process_batch(yuv[:2], annotate="inplace")
        finally:
            a.close()
            b.close()
        a, b = _pair(layout)
        try:
            ga = a.process_stream([yuv[:24], yuv[24:]], annotate=annotate)
            gb = b.process_stream([rgb[:24], rgb[24:]], annotate=annotate)
            for w, (oa, ob) in enumerate(zip(ga, gb)):
                if annotate:
                    assert len(oa) == 24 and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w
                else:
                    assert oa == ob == [None] * 24
            assert _state(a) == _state(b), annotate
            assert a.counter == 48
        finally:
            a.close()
            b.close()


def test_group_of_four_with_an_idle_stream():
    from lane_tracker_amd.group import LaneTrackerGroup
    cal = calib.reference_calibration()
    layout = "nv12"
    streams = [_stream(6, layout, 30 + i) for i in range(4)]
    ga, gb = LaneTrackerGroup(4, **cal, pixel_format=layout), LaneTrackerGroup(4, **cal)
    try:
        for tick in range(6):
            idle = tick % 4                            # one stream skips every call
            fa = [None if i == idle else streams[i][0][tick] for i in range(4)]
            fb = [None if i == idle else streams[i][1][tick] for i in range(4)]
            oa, ob = ga.process(fa), gb.process(fb)
            for i in range(4):
                assert (oa[i] is None) == (ob[i] is None) == (i == idle)
                if i != idle:
                    assert np.array_equal(oa[i], ob[i]), (tick, i)
                assert _state(ga.trackers[i]) == _state(gb.trackers[i]), (tick, i)
        assert sum(t.success for t in gb.trackers) * 10 >= sum(t.counter for t in gb.trackers) * 9
    finally:
        ga.close()
        gb.close()


def test_a_long_run_of_process_calls_keeps_device_memory_where_it_was():
    yuv, _ = _stream(10, "nv12", 5)
    a, _b = _pair("nv12")
    _b.close()
    try:
        for k in range(10):
            a.process(yuv[k % 10])
        live = _native.device_cache_stats()["live_bytes"]
        for k in range(200):
            a.process(yuv[k % 10])
        assert _native.device_cache_stats()["live_bytes"] == live
    finally:
        a.close()
