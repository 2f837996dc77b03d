"""Camera frames in packed YUV 4:2:2 (YUY2 / UYVY), converted on the device.  Everything here is bit for bit: the device conversion
is the integer formula `tests/yuv422_reference.py` restates, and everything behind it is the existing path -- so a 4:2:2 context or
tracker must give exactly what an RGB one gives on the converted frames.  There is no tolerance anywhere."""
import numpy as np
import pytest

import calibration_cameras as CC
import yuv422_reference as R
from lane_tracker_amd import _native, calib, synth
from lane_tracker_amd.device import DeviceBuffer, DeviceFrames, pack_host_frames
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

LAYOUTS = ("yuy2", "uyvy")
W, H = calib.IMAGE_WIDTH_HEIGHT


def _ctx(cal, capacity, pixel_format="rgb", matrix="bt601"):
    c = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                        capacity=capacity)
    if pixel_format != "rgb":
        c.set_input_format(pixel_format, matrix)
    return c


def _noise(seed, n=1, h=H, w=W):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 2), dtype=np.uint8)


def _to_rgb(frames, layout, matrix="bt601"):
    return np.stack([R.yuv422_to_rgb(f, layout, matrix) for f in frames])


def _surfaces(frames, layout, pitch=None, offset=0, fill=0xEE):
    """`frames` as pitched surfaces in a DeviceBuffer of their own that ends on the last byte of the last row; `fill` between rows."""
    block, surf, size, single = pack_host_frames(frames, layout, pitch=pitch, offset=offset, fill=fill)
    buf = DeviceBuffer(block.nbytes).copy_from_host(block)
    surf["plane"][:, :1] += np.uint64(buf.ptr)
    return DeviceFrames(surf, size, layout, owner=buf, single=single)


@pytest.fixture(scope="module")
def scenes():
    """Ten rendered scenes, RGB (shared; never changed)."""
    r = synth.SceneRenderer()
    out = np.stack([r.render(s)[0] for s in range(10)])
    out.setflags(write=False)
    return out


def _valid_lanes(records):
    """How many of the records show both lines detected and a lane check_validity accepts (an RGB tracker's own check)."""
    cal = calib.reference_calibration()
    t = LaneTracker(**cal)
    try:
        ok = 0
        for r in records:
            if r["detected"] and not r["fit_flags"]:
                t.check_validity(r["left_coeffs"], r["right_coeffs"])
                ok += bool(t.valid_lane_lines)
        return ok
    finally:
        t.close()


# ---- 1. the conversion itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 6), (66, 5), (1280, 720)], ids=lambda s: "%dx%d" % s)   # wide body; byte-wise body, odd height; a frame
@pytest.mark.parametrize("layout", LAYOUTS)
def test_yuv_to_rgb_is_the_restatement(layout, size):
    from lane_tracker_amd import utils
    w, h = size
    frame = _noise(h * 7 + w, 1, h, w)[0]          # uniform bytes: every clamp is hit
    for matrix in ("bt601", "bt709"):
        got = utils.yuv_to_rgb(frame, layout=layout, matrix=matrix)
        want = R.yuv422_to_rgb(frame, layout, matrix)
        assert got.shape == (h, w, 3) and got.dtype == np.uint8
        assert (want == 0).any() and (want == 255).any()
        assert np.array_equal(got, want), (matrix, np.argwhere(got != want)[:4])


# ---- 2. the walk on an identity camera: every row and column of the frame ----------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_walk_reads_every_byte_where_it_lies(layout):
    w, h = 64, 48
    mk = lambda: _native.Context((w, h), (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=4)
    frames = _noise(5, 3, h, w)
    want = _to_rgb(frames, layout)
    a = mk()
    try:
        a.set_input_format(layout)
        i = a.info()
        r0, r1 = i.src_row0, i.src_row1
        assert r0 == 0 and r1 >= h - 1                     # the bird's-eye view of this camera reads every row
        a.upload_frame_rows(frames, first=1)
        a.mask_run(3, first=1)
        und = a.download_undistorted(3, first=1)
        assert np.array_equal(und, want[:, r0:r1]), np.argwhere(und != want[:, r0:r1])[:4]
        planes = [a.download_plane(p, 3, first=1) for p in (0, 1)]
        # the same bytes as surfaces: pitch 2 W + {0, 1, 6}, base offset 0 .. 3, the plane ending on the last byte of its buffer
        for k, (extra, off) in enumerate(((0, 0), (1, 1), (6, 2), (1, 3), (0, 3))):
            b = mk()
            try:
                b.set_input_format(layout)
                dev = _surfaces(frames, layout, pitch=2 * w + extra, offset=off)
                assert int(dev.surfaces["plane"][0, 0]) % 4 == (dev.owner.ptr + off) % 4
                keep = b.attach_device_frames(dev, first=1)
                b.mask_run(3, first=1)
                assert np.array_equal(b.download_undistorted(3, first=1), und), (extra, off)
                for p in (0, 1):
                    assert np.array_equal(b.download_plane(p, 3, first=1), planes[p]), (extra, off, p)
                b.sync()
                del keep
            finally:
                b.close()
                dev.owner.close()
    finally:
        a.close()


# ---- 3. the mask chain of a 4:2:2 context = that of an RGB context given the converted frames ---------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_mask_chain_parity_with_an_rgb_context(layout, scenes):
    cal = calib.reference_calibration()
    cap = 22
    lanes = np.stack([R.rgb_to_yuv422(f, layout) for f in scenes])
    frames = np.concatenate([lanes, _noise(11, 10)])[[0, 10, 1, 11, 2, 12, 3, 13, 4, 14, 5, 15, 6, 16, 7, 17, 8, 18, 9, 19]]   # 20: mixed
    rgb = _to_rgb(frames, layout)
    a, b, d = _ctx(cal, cap, layout), _ctx(cal, cap), _ctx(cal, cap, layout)
    dev = _surfaces(frames, layout, pitch=2 * W + 6, offset=1)
    try:
        # the scenes must be ones a tracker FINDS lanes in, after the 4:2:2 round trip: asked of the RGB path before anything is compared
        b.upload_frame_rows(_to_rgb(lanes, layout))
        b.mask_run(10)
        b.sws_fit_run(10)
        assert _valid_lanes(b.download_records(10)) >= 9
        for n, first in ((1, 0), (1, 1), (2, 3), (3, 1), (16, 5)):
            rot = (n + first) % 7                                                       # other frames in the slots every time
            idx = np.roll(np.arange(len(frames)), rot)[:n]
            a.upload_frame_rows(frames[idx], first=first)
            b.upload_frame_rows(rgb[idx], first=first)
            part = DeviceFrames(dev.surfaces[idx], dev.img_size, layout, owner=dev.owner)
            keep = d.attach_device_frames(part, first=first)
            for c in (a, b, d):
                c.mask_run(n, first=first)
                c.sws_fit_run(n, first=first)
            for c, fed in ((a, "host"), (d, "attached")):
                what = "%s %s n=%d first=%d" % (layout, fed, n, first)
                assert np.array_equal(c.download_undistorted(n, first=first), b.download_undistorted(n, first=first)), what
                for plane in range(6):
                    assert np.array_equal(c.download_plane(plane, n, first=first), b.download_plane(plane, n, first=first)), (what, plane)
                assert np.array_equal(c.download_masks(n, first=first), b.download_masks(n, first=first)), what
                assert c.download_records(n, first=first).tobytes() == b.download_records(n, first=first).tobytes(), what
            d.sync()
            del keep
    finally:
        for c in (a, b, d):
            c.close()
        dev.owner.close()


# ---- 4. the RGB camera frame of a slot: the frame somebody shows -----------------------------------------------------------------
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


@pytest.mark.parametrize("layout", LAYOUTS)
def test_camera_frame_holds_the_converted_rows(layout, scenes):
    cal = calib.reference_calibration()
    frames = np.concatenate([_noise(21, 2), R.rgb_to_yuv422(scenes[3], layout)[None]])
    want = _to_rgb(frames, layout, "bt709")
    n = len(frames)
    c = _ctx(cal, 4, layout, "bt709")
    try:
        c.overlay_configure(cal["warp_matrices"][1])
        c.upload_frames(frames, first=1)                                             # the whole frame
        assert np.array_equal(_read_back(c, n, first=1), want), "lt_upload_frames"
        other, exp = np.roll(frames, 1, 0), np.roll(want, 1, 0)                       # rows + rest: the whole frame from two calls
        keep = [c.upload_frame_rows(other, first=1, enqueue=True)]
        c.mask_run(n, first=1)
        keep.append(c.upload_frame_rest(other, first=1))
        assert np.array_equal(_read_back(c, n, first=1), exp), "rows + rest"
        c.sync()
        # rows + rest_rows with two runs (odd bounds): those runs hold the new frame, every other row what it held (`exp`)
        r0, r1 = c.source_rows()
        third, exp3 = np.roll(frames, 2, 0), np.roll(want, 2, 0)
        runs = (5, 62, r0 + 9, H - 3)
        rows = np.array(runs, np.int32)
        keep = [c.upload_frame_rows(third, first=1, enqueue=True)]
        c.mask_run(n, first=1)
        keep.append(c.upload_frame_rest(third, first=1, rows=rows.ctypes.data))
        got = _read_back(c, n, first=1)
        held = exp.copy()
        for lo, hi in ((runs[0], runs[1]), (runs[2], runs[3])):
            held[:, lo:hi] = exp3[:, lo:hi]
        assert np.array_equal(got, held), ("rows + rest_rows", np.argwhere(got != held)[:4])
        c.sync()
        # attached surfaces: the whole frame, then two runs of another
        dev = _surfaces(frames, layout, pitch=2 * W + 6, offset=3)
        dev2 = _surfaces(other, layout)                                              # dense and aligned: the wide body
        try:
            keep = c.attach_device_frames(dev, first=1)
            c.mask_run(n, first=1)
            c.device_frames_rest(n, first=1)
            assert np.array_equal(_read_back(c, n, first=1), want), "attach + device_frames_rest"
            keep2 = c.attach_device_frames(dev2, first=1)
            c.mask_run(n, first=1)
            c.device_frames_rest(n, first=1, rows=rows.ctypes.data)
            got = _read_back(c, n, first=1)
            held = want.copy()
            for lo, hi in ((runs[0], runs[1]), (runs[2], runs[3])):
                held[:, lo:hi] = exp[:, lo:hi]
            assert np.array_equal(got, held), ("attach + device_frames_rest(rows4)", np.argwhere(got != held)[:4])
            c.sync()
            del keep, keep2
        finally:
            dev.owner.close()
            dev2.owner.close()
    finally:
        c.close()


# ---- 5. trackers: a 4:2:2 tracker = an RGB tracker on the converted frames, annotated frames included ---------------------------------
def _state(lt):
    b = lambda a: None if a is None else np.asarray(a).tobytes()
    return dict(detected=lt.detected_pixels, valid=lt.valid_lane_lines, last_detection=lt.last_detection, success=lt.success,
                counter=lt.counter, left_avg=b(lt.left_avg_coeffs), right_avg=b(lt.right_avg_coeffs), last_left=b(lt.last_left_coeffs),
                last_right=b(lt.last_right_coeffs), hist=[b(c) for c in lt.left_fit_coeffs] + [b(c) for c in lt.right_fit_coeffs],
                radii=list(lt.average_curve_radii), radius=lt.average_curve_radius, ecc=lt.eccentricity,
                pix=(b(lt.left_y), b(lt.left_x), b(lt.right_y), b(lt.right_x)), cent=(lt.left_window_centroids, lt.right_window_centroids))


@pytest.fixture(scope="module")
def lane_stream():
    """A drifting lane, 8 RGB frames (shared; never changed)."""
    out = synth.stream_lanes(8, seed=7)
    out.setflags(write=False)
    return out


def _stream(rgb, layout, blank=()):
    """The frames as 4:2:2 (and the RGB frames they convert to); `blank`: positions of black frames."""
    yuv = np.stack([R.rgb_to_yuv422(f, layout) for f in rgb])
    for k in blank:
        yuv[k] = R.pack_422(np.full((H, W), 16, np.uint8), np.full((H, W // 2), 128, np.uint8), np.full((H, W // 2), 128, np.uint8), layout)
    return yuv, _to_rgb(yuv, layout)


def _pair(layout):
    cal = calib.reference_calibration()
    return LaneTracker(**cal, pixel_format=layout), LaneTracker(**cal)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_trackers_equal_an_rgb_tracker_on_the_converted_frames(layout, lane_stream):
    yuv, rgb = _stream(lane_stream, layout)
    a, b = _pair(layout)
    try:
        for k in range(8):                                   # process()
            out_b = b.process(rgb[k])
            out_a = a.process(yuv[k])
            assert out_a.shape == (H, W, 3) and np.array_equal(out_a, out_b), k
            assert _state(a) == _state(b), k
        assert b.success >= 7, b.success                     # lanes were found
        sa, sb = a.get_state(), b.get_state()
        assert sa.pop("pixel_format") == layout and sa.pop("yuv_matrix") == "bt601" and sa == sb
        with pytest.raises(ValueError):
            a.process(rgb[5])
    finally:
        a.close()
        b.close()
    a, b = _pair(layout)
    try:                                                     # process_batch
        oa, ob = a.process_batch(yuv[:6]), b.process_batch(rgb[:6])
        assert len(oa) == 6 and all(np.array_equal(x, y) for x, y in zip(oa, ob))
        assert _state(a) == _state(b) and b.success >= 5
    finally:
        a.close()
        b.close()
    yuv, rgb = _stream(lane_stream, layout, blank=(5,))
    a, b = _pair(layout)
    try:                                                     # process_stream: two windows of 4, a blank frame in the second
        ga, gb = a.process_stream([yuv[:4], yuv[4:]]), b.process_stream([rgb[:4], rgb[4:]])
        for w, (oa, ob) in enumerate(zip(ga, gb)):
            assert len(oa) == 4 and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w
        assert _state(a) == _state(b) and a.counter == 8 and b.success >= 6
        a.warm(window=4)
    finally:
        a.close()
        b.close()


# ---- 6. a group of cameras with distinct calibrations: the table-per-slot forms ---------------------------------------------------
@pytest.mark.parametrize("fed", ["host", "device"])
def test_group_of_three_uyvy_cameras(fed):
    from lane_tracker_amd import LaneTrackerGroup
    cams = CC.cameras()
    names, k, n, layout = "ABE", 3, 6, "uyvy"
    rgb = [synth.stream_lanes(n, seed=5 + 13 * i) for i in range(k)]
    rgb[1] = CC.shifted(rgb[1])
    vids = [np.stack([R.rgb_to_yuv422(f, layout) for f in v]) for v in rgb]
    conv = [_to_rgb(v, layout) for v in vids]
    dev = [_surfaces(v, layout, pitch=2 * W + 6, offset=1) for v in vids] if fed == "device" else None
    g = LaneTrackerGroup(k, **cams["A"], pixel_format=layout, calibrations=[None, CC.overrides(cams["B"]), CC.overrides(cams["E"])])
    solos = [LaneTracker(**cams[x]) for x in names]          # RGB trackers, on the converted frames
    try:
        assert g.calibration_count() == 3
        pos = [0] * k
        for t in range(n):
            idle = t % k if t % 2 else None                  # one stream skips every other tick
            tick = [None if i == idle else (dev[i][pos[i]] if dev else vids[i][pos[i]]) for i in range(k)]
            outs = g.process(tick)
            for i in range(k):
                if i == idle:
                    assert outs[i] is None
                    continue
                want = solos[i].process(conv[i][pos[i]])
                assert np.array_equal(outs[i], want), (t, i)
                sg = g.trackers[i].get_state()
                assert sg.pop("pixel_format") == layout and sg.pop("yuv_matrix") == "bt601" and sg == solos[i].get_state(), (t, i)
                pos[i] += 1
        assert all(s.success > 0 for s in solos), [s.success for s in solos]
    finally:
        g.close()
        for s in solos:
            s.close()
        for d in dev or ():
            d.owner.close()


# ---- 7. refusals leave the context usable ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_refusals_leave_the_context_usable(layout, scenes):
    cal = calib.reference_calibration()
    k601 = np.array(_native.YUV_MATRICES["bt601"], np.int32)
    k8 = np.array(_native.RGB2YUV_MATRICES["bt601"], np.int32)
    code = _native.pixel_format_id(layout)
    odd = _native.Context((65, 34), (8, 8), np.eye(3), np.zeros(5), np.eye(3), capacity=1)
    try:
        with pytest.raises(ValueError):
            odd.set_input_format(layout)
        assert odd.lib.lt_set_input_format(odd._h, code, k601.ctypes.data) == -1      # LT_ERR_INVALID from the library itself
        assert odd.input_format()[0] == "rgb"
    finally:
        odd.close()
    tall = _native.Context((66, 35), (8, 8), np.eye(3), np.zeros(5), np.eye(3), capacity=1)      # an odd height is fine
    try:
        tall.set_input_format(layout)
        assert tall.input_format() == (layout, _native.YUV_MATRICES["bt601"])
    finally:
        tall.close()
    frames = np.stack([R.rgb_to_yuv422(f, layout) for f in scenes[:2]])
    c = _ctx(cal, 2, layout)
    dev = _surfaces(frames, layout)
    try:
        assert c.set_direct_upload(True) == 0                    # 4:2:2 rows take the engine
        c.overlay_configure(cal["warp_matrices"][1])
        c.upload_frame_rows(frames)
        c.mask_run(2)
        c.sws_fit_run(2)
        masks, recs = c.download_masks(2), c.download_records(2).tobytes()
        assert _valid_lanes(c.download_records(2)) == 2
        c.set_input_format(layout)                               # the same again is no change
        for other in ("rgb", "nv12", "uyvy" if layout == "yuy2" else "yuy2"):
            with pytest.raises(_native.NativeError):             # a change after an upload
                c.set_input_format(other)
        with pytest.raises(ValueError):
            c.upload_frame_rows(np.zeros((2, H, W, 3), np.uint8))
        short = DeviceFrames(dev.surfaces.copy(), dev.img_size, layout, owner=dev.owner)
        short.surfaces["pitch"] = 2 * W - 2
        with pytest.raises(ValueError):                          # LT_ERR_INVALID: a pitch below 2 W
            c.attach_device_frames(short)
        keep = c.attach_device_frames(dev)
        ok = np.zeros(2, np.int32)
        assert c.lib.lt_overlay_run_inplace(c._h, 0, 2, ok.ctypes.data, ok.ctypes.data, None, None, 0.3, None, k8.ctypes.data) == -5      # LT_ERR_STATE
        assert c.lib.lt_last_error()
        sink = DeviceFrames.empty(2, (W, H), "rgb")
        try:
            s = np.ascontiguousarray(sink.surfaces)
            for bad in (3, 4):
                assert c.lib.lt_overlay_store_device(c._h, 0, 2, s.ctypes.data, bad, k8.ctypes.data) == -1                                # LT_ERR_INVALID
        finally:
            sink.owner.close()
        # ... and the context works as before: the attached surfaces hold the same bytes
        c.mask_run(2)
        c.sws_fit_run(2)
        assert np.array_equal(c.download_masks(2), masks) and c.download_records(2).tobytes() == recs
        c.sync()
        del keep
    finally:
        c.close()
        dev.owner.close()
