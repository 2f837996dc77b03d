"""Camera frames and sinks in BGR, RGBA and BGRA.  The definition is a channel permutation -- `to_rgb` below, written out -- so a
context or tracker in one of these formats must give exactly what an RGB one gives on `to_rgb(frames)`, whatever the alpha bytes
hold, and a sink must hold exactly the permuted bytes with alpha 255.  Every comparison is equality; there is no tolerance."""
import numpy as np
import pytest

import calibration_cameras as CC
import sink_reference as S
from lane_tracker_amd import _native, calib, synth, utils
from lane_tracker_amd.device import DeviceBuffer, DeviceFrames, pack_host_frames
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

FORMATS = ("bgr", "rgba", "bgra")
BPP = {"bgr": 3, "rgba": 4, "bgra": 4}
W, H = calib.IMAGE_WIDTH_HEIGHT
FILL = 0xEE


def to_rgb(f, fmt):
    """The definition."""
    return np.ascontiguousarray({"bgr": lambda a: a[..., ::-1], "rgba": lambda a: a[..., :3], "bgra": lambda a: a[..., 2::-1]}[fmt](f))


def _pack(rgb, fmt, seed=0):
    """RGB frames in `fmt`, every alpha byte random."""
    out = utils.rgb_to_packed(rgb, fmt)
    if BPP[fmt] == 4:
        out[..., 3] = np.random.default_rng(seed).integers(0, 256, out.shape[:-1], dtype=np.uint8)
    assert np.array_equal(to_rgb(out, fmt), rgb)
    return out


def _noise(seed, fmt, n=1, h=H, w=W):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, BPP[fmt]), dtype=np.uint8)


def _ctx(cal, capacity, fmt="rgb"):
    c = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], capacity=capacity)
    if fmt != "rgb":
        c.set_input_format(fmt)
    return c


def _identity(w, h, fmt="rgb", capacity=4):
    c = _native.Context((w, h), (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=capacity)
    if fmt != "rgb":
        c.set_input_format(fmt)
    return c


def _surfaces(frames, fmt, pitch=None, offset=0, fill=FILL):
    """`frames` as pitched surfaces in a DeviceBuffer of their own that ends on the last byte of the last row; `fill` between rows."""
    block, surf, size, single = pack_host_frames(frames, fmt, pitch=pitch, offset=offset, fill=fill)
    buf = DeviceBuffer(block.nbytes).copy_from_host(block)
    surf["plane"][:, :1] += np.uint64(buf.ptr)
    return DeviceFrames(surf, size, fmt, owner=buf, single=single)


@pytest.fixture(scope="module")
def scenes():
    """Four rendered scenes, RGB (shared; never changed)."""
    r = synth.SceneRenderer()
    out = np.stack([r.render(s)[0] for s in range(4)])
    out.setflags(write=False)
    return out


def _valid_lanes(records):
    """How many of the records show both lines detected and a lane check_validity accepts (an RGB tracker's own check)."""
    t = LaneTracker(**calib.reference_calibration())
    try:
        ok = 0
        for r in records:
            if r["detected"] and not r["fit_flags"]:
                t.check_validity(r["left_coeffs"], r["right_coeffs"])
                ok += bool(t.valid_lane_lines)
        return ok
    finally:
        t.close()


def _front(c, n, first=0):
    """What the front end left for slots [first, first + n): the undistorted rows and the two planes the warp emits."""
    c.mask_run(n, first=first)
    return [c.download_undistorted(n, first=first), c.download_plane(0, n, first=first), c.download_plane(1, n, first=first)]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. + 3. the walk on an identity camera: every byte where it lies, from slots and from surfaces ---------------------------------
@pytest.mark.parametrize("size", [(64, 48), (66, 50), (37, 21), (2, 2)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", FORMATS)
def test_walk_reads_every_byte_where_it_lies(fmt, size):
    """(66, 50): 24-bit rows that are no multiple of 4 bytes; (37, 21): odd in both; (2, 2): the narrowest frame, the window's column
    clamps to 0.  Surfaces at pitch row + 5 and base offsets 0 .. 3: every byte alignment of the window, rows of the 32-bit formats
    that are not dword-aligned, and a surface that ends on the last byte of its allocation."""
    w, h = size
    frames = _noise(5 + w, fmt, 3, h, w)                       # random alpha
    a, b = _identity(w, h, fmt), _identity(w, h)
    try:
        a.upload_frame_rows(frames, first=1)
        b.upload_frame_rows(to_rgb(frames, fmt), first=1)
        want = _front(b, 3, first=1)
        assert want[0].size and _same(_front(a, 3, first=1), want)
        row = BPP[fmt] * w
        for off in range(4):
            d = _identity(w, h, fmt)
            dev = _surfaces(frames, fmt, pitch=row + 5, offset=off)
            try:
                assert int(dev.surfaces["plane"][0, 0]) == dev.owner.ptr + off
                keep = d.attach_device_frames(dev, first=1)
                assert _same(_front(d, 3, first=1), want), off
                d.sync()
                del keep
            finally:
                d.close()
                dev.owner.close()
        # a range that mixes attached and plain slots: slot 2 reads a surface, slots 1 and 3 their own staging frames
        other = _noise(77 + w, fmt, 1, h, w)
        dev = _surfaces(other, fmt, pitch=row + 5, offset=1)
        try:
            keep = a.attach_device_frames(dev, first=2)
            b.upload_frame_rows(to_rgb(other, fmt), first=2)
            assert _same(_front(a, 3, first=1), _front(b, 3, first=1))
            a.sync()
            del keep
        finally:
            dev.owner.close()
    finally:
        a.close()
        b.close()


# ---- 2. out-of-frame taps and fractions: the reference calibration ------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_mask_chain_parity_with_an_rgb_context(fmt, scenes):
    cal = calib.reference_calibration()
    frames = np.concatenate([_pack(scenes, fmt, seed=3), _noise(11, fmt, 4)])
    rgb = to_rgb(frames, fmt)
    n = len(frames)
    a, b, d = _ctx(cal, n, fmt), _ctx(cal, n), _ctx(cal, n, fmt)
    dev = _surfaces(frames, fmt, pitch=BPP[fmt] * W + 5, offset=1)
    try:
        a.upload_frame_rows(frames)
        b.upload_frame_rows(rgb)
        keep = d.attach_device_frames(dev)
        for c in (a, b, d):
            c.mask_run(n)
            c.sws_fit_run(n)
        assert _valid_lanes(b.download_records(n)) >= 2
        for c, fed in ((a, "host"), (d, "attached")):
            assert np.array_equal(c.download_undistorted(n), b.download_undistorted(n)), fed
            for plane in range(6):
                assert np.array_equal(c.download_plane(plane, n), b.download_plane(plane, n)), (fed, plane)
            assert np.array_equal(c.download_masks(n), b.download_masks(n)), fed
            assert c.download_records(n).tobytes() == b.download_records(n).tobytes(), fed
        d.sync()
        del keep
        # lt_mask_batch takes such frames
        import ctypes as C
        f3, want3, fp = np.ascontiguousarray(frames[:3]), b.download_masks(3), _native.filter_params()
        got3 = np.zeros_like(want3)
        assert a.lib.lt_mask_batch(a._h, f3.ctypes.data, 3, C.byref(fp), got3.ctypes.data) == 0
        assert np.array_equal(got3, want3)
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


@pytest.mark.parametrize("fmt", FORMATS)
def test_camera_frame_holds_the_rgb_rows(fmt, scenes):
    cal = calib.reference_calibration()
    frames = np.concatenate([_noise(21, fmt, 2), _pack(scenes[3:4], fmt, seed=8)])
    want = to_rgb(frames, fmt)
    n = len(frames)
    c = _ctx(cal, 4, fmt)
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
        # the list forms: frames that lie in separate host arrays
        sep = [np.ascontiguousarray(f) for f in frames]
        keep = [c.upload_frame_rows_list(sep, first=1)]
        c.mask_run(n, first=1)
        keep.append(c.upload_frame_rest_list(sep, first=1))
        assert np.array_equal(_read_back(c, n, first=1), want), "the list forms"
        c.sync()
        # attached surfaces: the whole frame (byte-wise body), then two runs of another (dense and aligned: the wide body)
        dev = _surfaces(other, fmt, pitch=BPP[fmt] * W + 5, offset=3)
        dev2 = _surfaces(third, fmt)
        try:
            keep = c.attach_device_frames(dev, first=1)
            c.mask_run(n, first=1)
            c.device_frames_rest(n, first=1)
            assert np.array_equal(_read_back(c, n, first=1), exp), "attach + device_frames_rest"
            keep2 = c.attach_device_frames(dev2, first=1)
            c.mask_run(n, first=1)
            c.device_frames_rest(n, first=1, rows=rows.ctypes.data)
            got = _read_back(c, n, first=1)
            held = exp.copy()
            for lo, hi in ((runs[0], runs[1]), (runs[2], runs[3])):
                held[:, lo:hi] = exp3[:, lo:hi]
            assert np.array_equal(got, held), ("attach + device_frames_rest(rows4)", np.argwhere(got != held)[:4])
            c.sync()
            del keep, keep2
        finally:
            dev.owner.close()
            dev2.owner.close()
    finally:
        c.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_camera_frame_of_an_odd_width(fmt):
    """The byte-wise body from a slot's staging frame (37 x 21: no wide body), read back as the whole frame."""
    w, h = 37, 21
    frames = _noise(31, fmt, 2, h, w)
    c = _identity(w, h, fmt)
    try:
        c.overlay_configure(np.eye(3))
        c.upload_frames(frames)
        e = np.zeros(0, np.int64)
        c.overlay_run([(e, e, e, e)] * 2)
        assert np.array_equal(c.download_overlay(2), to_rgb(frames, fmt))
    finally:
        c.close()


# ---- 5. trackers -----------------------------------------------------------------------------------------------------------------
def _state(lt):
    b = lambda a: None if a is None else np.asarray(a).tobytes()
    return dict(detected=lt.detected_pixels, valid=lt.valid_lane_lines, last_detection=lt.last_detection, success=lt.success,
                counter=lt.counter, left_avg=b(lt.left_avg_coeffs), right_avg=b(lt.right_avg_coeffs), last_left=b(lt.last_left_coeffs),
                last_right=b(lt.last_right_coeffs), hist=[b(c) for c in lt.left_fit_coeffs] + [b(c) for c in lt.right_fit_coeffs],
                radii=list(lt.average_curve_radii), radius=lt.average_curve_radius, ecc=lt.eccentricity,
                pix=(b(lt.left_y), b(lt.left_x), b(lt.right_y), b(lt.right_x)), cent=(lt.left_window_centroids, lt.right_window_centroids))


N_STREAM, BLANK, HALF = 40, (17, 18, 31), 20


def _tracker_runs(stream, fmt):
    """A stream through every way a tracker takes frames -> {what: (the frames it returned, its state, its success ratio)}."""
    cal = calib.reference_calibration()
    kw = {} if fmt == "rgb" else dict(pixel_format=fmt)
    runs = {}

    def run(what, fn):
        t = LaneTracker(**cal, **kw)
        try:
            out = fn(t)
            st = t.get_state()
            assert st.pop("pixel_format", fmt) == fmt
            st.pop("yuv_matrix", None)
            runs[what] = (out, _state(t), st, t.get_success_ratio())
        finally:
            t.close()
    cp = lambda o: None if o is None else tuple(np.array(x) for x in o) if isinstance(o, tuple) else np.array(o)
    run("process", lambda t: [cp(t.process(f)) for f in stream])
    run("batch", lambda t: [cp(o) for o in t.process_batch(stream)])
    run("stream", lambda t: [cp(o) for win in t.process_stream([stream[:HALF], stream[HALF:]]) for o in win])
    run("stream_plain", lambda t: [cp(o) for win in t.process_stream([stream[:HALF], stream[HALF:]], annotate=False) for o in win])
    run("viz", lambda t: [cp(t.process(f, visualize_search=True)) for f in stream])
    run("split", lambda t: [cp(t.process(f, split_view=True)) for f in stream])
    run("batch_viz", lambda t: [cp(o) for o in t.process_batch(stream[:HALF], visualize_search=True)])
    run("batch_split", lambda t: [cp(o) for o in t.process_batch(stream[:HALF], split_view=True)])
    return runs


@pytest.fixture(scope="module")
def lane_stream():
    """A drifting lane with a few blank frames, RGB (shared; never changed), and what an RGB tracker makes of it."""
    rgb = synth.stream_lanes(N_STREAM, seed=7).copy()
    rgb[list(BLANK)] = 0
    rgb.setflags(write=False)
    return rgb, _tracker_runs(rgb, "rgb")


def _equal(x, y):
    if x is None or y is None:
        return x is None and y is None
    if isinstance(x, tuple):
        return isinstance(y, tuple) and len(x) == len(y) and all(_equal(p, q) for p, q in zip(x, y))
    return x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.parametrize("fmt", FORMATS)
def test_trackers_equal_an_rgb_tracker(fmt, lane_stream):
    rgb, want = lane_stream
    assert want["process"][3][1] >= N_STREAM // 2, want["process"][3]                            # lanes were found
    got = _tracker_runs(_pack(rgb, fmt, seed=5), fmt)
    assert sorted(got) == sorted(want)
    for what in want:
        (oa, sa, ga, ra), (ob, sb, gb, rb) = got[what], want[what]
        assert len(oa) == len(ob) and all(_equal(x, y) for x, y in zip(oa, ob)), what
        assert sa == sb and ra == rb, what
        assert ga == gb, what
    t = LaneTracker(**calib.reference_calibration(), pixel_format=fmt)
    try:
        t.warm(window=4)
        with pytest.raises(ValueError):
            t.process(np.zeros((H, W, 7 - BPP[fmt]), np.uint8))
    finally:
        t.close()


@pytest.mark.parametrize("fed", ["host", "device"])
def test_group_of_three_bgra_cameras(fed):
    """Two distinct calibrations among three streams: the table-per-slot forms of the walk, from slots and from surfaces."""
    from lane_tracker_amd import LaneTrackerGroup
    cams = CC.cameras()
    names, k, n, fmt = "ABA", 3, 6, "bgra"
    rgb = [synth.stream_lanes(n, seed=5 + 13 * i) for i in range(k)]
    rgb[1] = CC.shifted(rgb[1])
    vids = [_pack(v, fmt, seed=i) for i, v in enumerate(rgb)]
    dev = [_surfaces(v, fmt, pitch=4 * W + 5, offset=1) for v in vids] if fed == "device" else None
    g = LaneTrackerGroup(k, **cams["A"], pixel_format=fmt, calibrations=[None, CC.overrides(cams["B"]), None])
    solos = [LaneTracker(**cams[x]) for x in names]          # RGB trackers, on to_rgb(frames)
    try:
        assert g.calibration_count() == 2
        pos = [0] * k
        for t in range(n):
            idle = t % k if t % 2 else None                  # one stream skips every other tick
            tick = [None if i == idle else (dev[i][pos[i]] if dev else vids[i][pos[i]]) for i in range(k)]
            outs = g.process(tick)
            for i in range(k):
                if i == idle:
                    assert outs[i] is None
                    continue
                want = solos[i].process(rgb[i][pos[i]])
                assert np.array_equal(outs[i], want), (t, i)
                sg = g.trackers[i].get_state()
                assert sg.pop("pixel_format") == fmt
                sg.pop("yuv_matrix")
                assert sg == solos[i].get_state(), (t, i)
                pos[i] += 1
        assert all(s.success > 0 for s in solos), [s.success for s in solos]
    finally:
        g.close()
        for s in solos:
            s.close()
        for d in dev or ():
            d.owner.close()


# ---- 6. sinks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 48), (37, 21), (1, 1)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", FORMATS)
def test_rgb_to_surfaces_writes_the_permuted_bytes_and_nothing_else(fmt, size):
    w, h = size
    n = 2
    rgb = np.random.default_rng(w * 7 + h).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    want_frames = utils.rgb_to_packed(rgb, fmt)                                        # alpha 255
    row = BPP[fmt] * w
    with DeviceBuffer(rgb.nbytes) as src:
        src.copy_from_host(rgb)
        for extra in (0, 5, 37):
            for off in range(4):
                sink = DeviceFrames.empty(n, (w, h), fmt, pitch=row + extra, offset=off, fill=FILL)
                try:
                    _native.rgb_to_surfaces(src.ptr, h * w * 3, (w, h), sink)
                    want = pack_host_frames(want_frames, fmt, pitch=row + extra, offset=off, fill=FILL)[0]
                    got = sink.owner.copy_to_host()
                    # the pixels are the permuted bytes, and every byte before, between and behind the rows keeps the sentinel
                    assert got.shape == want.shape and np.array_equal(got, want), (extra, off, np.argwhere(got != want)[:4])
                    assert np.array_equal(sink.to_host(), want_frames)
                finally:
                    sink.owner.close()


def test_process_batch_into_sinks_of_the_family(scenes):
    """An RGB tracker into a 'bgra' sink (pitched) and a 'bgr' sink (dense, 16-byte aligned: the wide body), and a 'bgr' tracker
    into an 'nv12' sink: the conversions of the RGB tracker's host frames."""
    cal = calib.reference_calibration()
    rgb = np.ascontiguousarray(scenes[:3])
    n = len(rgb)
    a, b, c = LaneTracker(**cal), LaneTracker(**cal), LaneTracker(**cal, pixel_format="bgr")
    sinks = [DeviceFrames.empty(n, (W, H), "bgra", pitch=4 * W + 5, offset=1, fill=FILL), DeviceFrames.empty(n, (W, H), "bgr", fill=FILL),
             DeviceFrames.empty(n, (W, H), "nv12", fill=FILL), DeviceFrames.empty(n, (W, H), "rgba", fill=FILL)]
    try:
        want = np.stack(a.process_batch(rgb))
        assert a.success >= 2
        got = b.process_batch(rgb, out=sinks[0])
        assert len(got) == n and np.array_equal(sinks[0].to_host(), utils.rgb_to_packed(want, "bgra"))
        raw = sinks[0].owner.copy_to_host()
        assert np.array_equal(raw, pack_host_frames(utils.rgb_to_packed(want, "bgra"), "bgra", pitch=4 * W + 5, offset=1, fill=FILL)[0])
        b2 = LaneTracker(**cal)
        try:
            b2.process_batch(rgb, out=sinks[1])
            assert np.array_equal(sinks[1].to_host(), utils.rgb_to_packed(want, "bgr"))
            for win in b2.process_stream([rgb], out=[sinks[3]]):
                assert len(win) == n
            assert np.array_equal(sinks[3].to_host(), utils.rgb_to_packed(np.stack(a.process_batch(rgb)), "rgba"))
        finally:
            b2.close()
        c.process_batch(_pack(rgb, "bgr"), out=sinks[2])
        assert np.array_equal(sinks[2].to_host(), np.stack([S.rgb_to_yuv420(f, "nv12") for f in want]))
    finally:
        for t in (a, b, c):
            t.close()
        for s in sinks:
            s.owner.close()


# ---- 7. refusals leave the context usable ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_refusals_leave_the_context_usable(fmt, scenes):
    cal = calib.reference_calibration()
    k8 = np.array(_native.RGB2YUV_MATRICES["bt601"], np.int32)
    code = _native.pixel_format_id(fmt)
    with pytest.raises(ValueError):                                                  # width 1: no context has it (LT_ERR_INVALID from lt_create) ...
        _native.Context((1, 34), (8, 8), np.eye(3), np.zeros(5), np.eye(3), capacity=1)
    with pytest.raises(ValueError):                                                  # ... and no tracker in these formats
        LaneTracker(**dict(cal, img_size=(1, H)), pixel_format=fmt)
    thin = _native.Context((2, 34), (8, 8), np.eye(3), np.zeros(5), np.eye(3), capacity=1)
    try:
        assert thin.lib.lt_set_input_format(thin._h, 8, None) == -1                  # no such layout: LT_ERR_INVALID
        assert thin.input_format()[0] == "rgb"
        thin.set_input_format(fmt)                                                   # the narrowest frame is fine
        assert thin.input_format()[0] == fmt
    finally:
        thin.close()
    sized = _ctx(cal, 1)
    try:
        sized.set_input_size((W // 2, H // 2))
        assert sized.lib.lt_set_input_format(sized._h, code, None) == -5             # LT_ERR_STATE: these frames are not resized
        assert sized.input_format()[0] == "rgb"
    finally:
        sized.close()
    frames = _pack(scenes[:2], fmt, seed=2)
    c = _ctx(cal, 2, fmt)
    dev = _surfaces(frames, fmt)
    try:
        assert c.input_format()[0] == fmt
        assert c.set_direct_upload(True) == 0                    # the rows go to staging
        c.overlay_configure(cal["warp_matrices"][1])
        c.upload_frame_rows(frames)
        c.mask_run(2)
        c.sws_fit_run(2)
        masks, recs = c.download_masks(2), c.download_records(2).tobytes()
        assert _valid_lanes(c.download_records(2)) == 2

        def unchanged(what):
            c.mask_run(2)
            c.sws_fit_run(2)
            assert np.array_equal(c.download_masks(2), masks) and c.download_records(2).tobytes() == recs, what
        c.set_input_format(fmt)                                  # the same again is no change
        for other in ("rgb", "nv12", "yuy2") + tuple(f for f in FORMATS if f != fmt):
            with pytest.raises(_native.NativeError):             # a change after an upload
                c.set_input_format(other)
        assert c.lib.lt_set_input_format(c._h, 8, None) == -1    # layout 8: LT_ERR_INVALID
        unchanged("format change")
        with pytest.raises(ValueError):
            c.upload_frame_rows(np.zeros((2, H, W, 7 - BPP[fmt]), np.uint8))
        assert c.lib.lt_set_input_size(c._h, W // 2, H // 2) == -5                    # LT_ERR_STATE
        unchanged("lt_set_input_size")
        short = DeviceFrames(dev.surfaces.copy(), dev.img_size, fmt, owner=dev.owner)
        short.surfaces["pitch"] = BPP[fmt] * W - 1
        with pytest.raises(ValueError):                          # LT_ERR_INVALID: a pitch below a row
            c.attach_device_frames(short)
        s_ = np.ascontiguousarray(short.surfaces)
        assert c.lib.lt_attach_device_frames(c._h, s_.ctypes.data, 0, 2) == -1
        unchanged("attach with a short pitch")
        keep = c.attach_device_frames(dev)
        ok = np.zeros(2, np.int32)
        assert c.lib.lt_overlay_run_inplace(c._h, 0, 2, ok.ctypes.data, ok.ctypes.data, None, None, 0.3, None, k8.ctypes.data) == -5      # LT_ERR_STATE
        assert c.lib.lt_last_error()
        unchanged("lt_overlay_run_inplace")                      # (the attached surfaces hold the same bytes)
        sink = DeviceFrames.empty(2, (W, H), fmt)
        try:
            s = np.ascontiguousarray(sink.surfaces)
            e = np.zeros(0, np.int64)
            assert c.lib.lt_overlay_run_to_surfaces(c._h, 0, 2, ok.ctypes.data, ok.ctypes.data, None, None, 0.3, None, s.ctypes.data, code, None) == -1
            assert c.lib.lt_overlay_store_device(c._h, 0, 2, s.ctypes.data, 8, None) == -1
            c.device_frames_rest(2)
            c.overlay_run([(e, e, e, e)] * 2)
            c.store_overlay_device(sink)                         # ... while the store into such a sink is fine
            c.store_wait()
            assert np.array_equal(to_rgb(sink.to_host(), fmt), to_rgb(frames, fmt))
        finally:
            sink.owner.close()
        unchanged("sinks")
        c.sync()
        del keep
    finally:
        c.close()
        dev.owner.close()
