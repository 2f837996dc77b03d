"""Camera frames in 8-bit raw Bayer (RGGB / GRBG / GBRG / BGGR), demosaiced on the device.  Everything here is bit for bit: the device
demosaic is the integer formula `tests/bayer_reference.py` restates, and everything behind it is the existing path -- so a raw Bayer
context or tracker must give exactly what the oracle, or an RGB tracker, gives on the demosaiced frames.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import bayer_reference as RB
import calibration_cameras as CC
import front_matrix as FM
from lane_tracker_amd import _native, calib, synth, utils
from lane_tracker_amd.device import DeviceBuffer, DeviceFrames, pack_host_frames
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

PATTERNS = RB.PATTERNS
W, H = calib.IMAGE_WIDTH_HEIGHT
SOURCES = ("host", "rows", "surfaces")
POOL = 8                                 # frames of a case's pool


# ---- the front-end matrix -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool(pattern, size):
    w, h = FM.SIZES[size]
    out = np.random.default_rng(7000 + 16 * "AB".index(size) + PATTERNS.index(pattern)).integers(0, 256, (POOL, h, w), dtype=np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(pattern, size, s, k):
    """Frame k of the case's pool, demosaiced by the restatement, through set s of the size -> (undistorted image, R plane, Lab-b
    plane) of the oracle, once."""
    O, oc = FM._oracle(), FM.oracle_calib(size, s)
    rgb = RB.bayer_to_rgb(_pool(pattern, size)[k], pattern)
    bev = O.front_end(oc, rgb)
    out = (O.undistort(oc, rgb), np.ascontiguousarray(bev[..., 0]), O.lab_b(bev))
    for a in out:
        a.setflags(write=False)
    return out


def _context(pattern, size, own, capacity, add=()):
    """A raw Bayer context of the size whose own calibration is set `own`, with the sets `add` added."""
    sets = FM.calibration_sets(size)
    q = sets[own]
    c = _native.Context(FM.SIZES[size], FM.SIZES[size], q["cam_matrix"], q["dist_coeffs"], q["M"], capacity=capacity)
    try:
        c.set_input_format(pattern)
        assert c.input_format()[0] == pattern
        for s in add:
            c.add_calibration(sets[s]["cam_matrix"], sets[s]["dist_coeffs"], sets[s]["M"])
        c.set_streams(1)
    except BaseException:
        c.close()
        raise
    return c


def _feed(ctx, pattern, size, frames, first, source, offset):
    """The frames into slots first, ...: whole frames from the host, the row run the path reads from the host, or pitched surfaces
    (pitch W + 5, the block ending on the last byte of the last row) -- the slot's own staging frame then holds the complement.
    -> the DeviceFrames that must outlive the run (or None)."""
    if source == "host":
        ctx.upload_frames(frames, first=first)
        return None
    ctx.upload_frames(~frames, first=first)                  # what a walk that reads the wrong rows or the wrong source would show
    if source == "rows":
        ctx.upload_frame_rows(frames, first=first)
        return None
    dev = FM.device_surfaces(frames, pattern, size, offset)
    try:
        assert int(dev.surfaces["plane"][0, 0]) == dev.owner.ptr + offset and int(dev.surfaces["pitch"][0]) == FM.SIZES[size][0] + 5
        ctx.attach_device_frames(dev, first=first)
    except BaseException:
        dev.owner.close()
        raise
    return dev


def _differing(got, want):
    d = got != want
    return int((d.any(-1) if d.ndim == 3 else d).sum())


def _run_and_compare(ctx, pattern, size, ids, first, source, shift, offset, where):
    """Slot first + i takes frame (i + shift) % POOL of the pool and set ids[i]; undistorted rows, R plane and Lab-b plane of every
    slot against the oracle."""
    n = len(ids)
    ks = [(i + shift) % POOL for i in range(n)]
    dev = _feed(ctx, pattern, size, np.ascontiguousarray(_pool(pattern, size)[ks]), first, source, offset)
    try:
        ctx.mask_run(n, first=first)
        und = ctx.download_undistorted(n, first=first)
        got_r, got_b = ctx.download_plane(0, n, first=first), ctx.download_plane(1, n, first=first)
        ctx.sync()
    finally:
        if dev is not None:
            dev.owner.close()
    i0, i1 = ctx.info().src_row0, ctx.info().src_row1
    for i, (k, s) in enumerate(zip(ks, ids)):
        want_u, want_r, want_b = _reference(pattern, size, s, k)
        msg = "%s, source %s, slot %d, set %d (frame %d of the pool): " % (where, source, first + i, s, k)
        assert np.array_equal(und[i], want_u[i0:i1]), msg + "%d undistorted pixels differ in rows [%d, %d)" % (_differing(und[i], want_u[i0:i1]), i0, i1)
        assert np.array_equal(got_r[i], want_r), msg + "%d pixels of the R plane differ" % _differing(got_r[i], want_r)
        assert np.array_equal(got_b[i], want_b), msg + "%d pixels of the Lab-b plane differ" % _differing(got_b[i], want_b)


@pytest.mark.parametrize("size", ["A", "B"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_front_end_equals_the_oracle(pattern, size):
    """4 patterns x sizes A (64 x 48) and B (66 x 50: row bytes and bird's-eye width no multiples of 4) x the four calibration sets
    (identity, taps outside the image, a narrow run of camera rows, general affine) x sources (host upload, row-run upload, surfaces
    at pitch W + 5 with odd offsets) x table forms (the shared table: a context per set; table-per-slot with ids_pattern)."""
    w, h = FM.SIZES[size]
    case = 0
    for s in range(FM.N_SETS):                               # the shared table: the context's own set is s
        ctx = _context(pattern, size, s, 4)
        try:
            r0, r1 = ctx.info().src_row0, ctx.info().src_row1
            assert (r0, r1) == tuple(FM.source_rows(size, s))
            c0, c1 = ctx.source_rows()
            i0, i1 = ctx.input_rows()                         # what a row-run upload moves: the run widened for the 3 x 3 support and the clamp
            assert (i0, i1) == (min(max(c0 - 1, 0), h - 4), min(max(c1 + 1, min(max(c0 - 1, 0), h - 4) + 4), h)), (c0, c1, i0, i1)
            if s == 2:
                assert c1 - c0 < h and (i0, i1) != (c0, c1)   # the narrow run
            for source in SOURCES:
                case += 1
                _run_and_compare(ctx, pattern, size, [s] * 3, 1, source, case, case % 4, "%s %s (%dx%d), shared table of set %d" % (pattern, size, w, h, s))
        finally:
            ctx.close()
    ids = FM.ids_pattern(5)                                  # table-per-slot: every set among five slots from an odd first slot
    assert set(ids) == set(range(FM.N_SETS))
    ctx = _context(pattern, size, 0, 6, add=(1, 2, 3))
    try:
        assert (ctx.info().src_row0, ctx.info().src_row1) == (0, h)          # the identity's rows: the whole image
        for source in SOURCES:
            case += 1
            ctx.set_slot_calibrations(ids, first=1)
            assert list(ctx.slot_calibrations(len(ids), first=1)) == ids
            _run_and_compare(ctx, pattern, size, ids, 1, source, case, case % 4, "%s %s (%dx%d), table per slot" % (pattern, size, w, h))
    finally:
        ctx.close()


# ---- the smallest frames --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(4, 4), (6, 4)])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_smallest_frames(pattern, w, h):
    """A 4 x 4 context -- the window is the whole plane, every tap is clamped -- and a 6 x 4 one, under a distortion that throws taps
    outside on every side: the undistorted rows, from the host, from a row-run upload and from surfaces."""
    K = np.array([[2.0, 0, (w - 1) / 2], [0, 2.0, (h - 1) / 2], [0, 0, 1.0]])
    dist, M = np.array([0.3, 0, 0, 0, 0.0]), np.diag([64 / w, 48 / h, 1.0])
    O = FM._oracle()
    oc = O.make_calib((w, h), (64, 48), K, dist, M)
    xy, _ = O.undistort_map(oc)
    sx, sy = xy[..., 0].astype(int), xy[..., 1].astype(int)
    assert sx.min() < 0 and sx.max() + 1 > w - 1 and sy.min() < 0 and sy.max() + 1 > h - 1      # taps outside on every side
    assert tuple(O.warp_source_rows(oc)) == (0, h)
    frames = np.random.default_rng(w * 10 + PATTERNS.index(pattern)).integers(0, 256, (3, h, w), dtype=np.uint8)
    want = np.stack([O.undistort(oc, RB.bayer_to_rgb(f, pattern)) for f in frames])
    ctx = _native.Context((w, h), (64, 48), K, dist, M, capacity=4)
    try:
        ctx.set_input_format(pattern)
        assert ctx.input_rows() == (0, h)
        for source in SOURCES:
            dev = None
            if source == "host":
                ctx.upload_frames(frames, first=1)
            elif source == "rows":
                ctx.upload_frames(~frames, first=1)
                ctx.upload_frame_rows(frames, first=1)
            else:
                ctx.upload_frames(~frames, first=1)
                block, surf, _, _ = pack_host_frames(frames, pattern, pitch=w + 5, offset=3, fill=0xEE)
                buf = DeviceBuffer(block.nbytes).copy_from_host(block)
                surf["plane"][:, :1] += np.uint64(buf.ptr)
                dev = DeviceFrames(surf, (w, h), pattern, owner=buf)
                ctx.attach_device_frames(dev, first=1)
            try:
                ctx.mask_run(3, first=1)
                und = ctx.download_undistorted(3, first=1)
                ctx.sync()
            finally:
                if dev is not None:
                    dev.owner.close()
            assert np.array_equal(und, want), (pattern, w, h, source, np.argwhere(und != want)[:4])
    finally:
        ctx.close()


# ---- the row conversion ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 48), (66, 50), (6, 4)], ids=lambda s: "%dx%d" % s)    # the 16-column body; the byte-wise body; the smallest
@pytest.mark.parametrize("pattern", PATTERNS)
def test_bayer_to_rgb_is_the_restatement(pattern, size):
    w, h = size
    frames = np.random.default_rng(h * 7 + w).integers(0, 256, (2, h, w), dtype=np.uint8)
    frames[1, :, : w // 2] = 255                             # a saturated half: the sums' largest values
    got = utils.bayer_to_rgb(frames, pattern)
    want = RB.bayer_to_rgb(frames, pattern)
    assert got.shape == (2, h, w, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(utils.bayer_to_rgb(frames[0], pattern), want[0])


def _read_back(c, n, h, w, first=0):
    """Every row of the camera frames of slots [first, first + n) through the overlay with no points (a plain copy) over two runs of
    rows that cover the frame."""
    e = np.zeros(0, np.int64)
    rows = np.array([0, h // 2, h // 2, h], np.int32)
    c.overlay_run([(e, e, e, e)] * n, first=first, rows=rows.ctypes.data)
    out = _native.pinned_empty((n, h, w, 3))
    out[:] = 0
    c.download_overlay_async(out, first=first, rows=rows.ctypes.data)
    c.sync()
    return np.array(out)


def _surfaces(frames, pattern, pitch=None, offset=0):
    block, surf, size, single = pack_host_frames(frames, pattern, pitch=pitch, offset=offset, fill=0xEE)
    buf = DeviceBuffer(block.nbytes).copy_from_host(block)
    surf["plane"][:, :1] += np.uint64(buf.ptr)
    return DeviceFrames(surf, size, pattern, owner=buf, single=single)


@pytest.mark.parametrize("size", [(64, 48), (66, 50), (6, 4)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_camera_frame_holds_the_demosaiced_rows(pattern, size):
    """The frame somebody shows: whole uploads, rows + rest, rows + rest over two runs that start and end on odd rows, attached
    surfaces at an unaligned pitch (and dense ones: the 16-column body) with lt_device_frames_rest, whole and over the two runs."""
    w, h = size
    frames = np.random.default_rng(31 + w).integers(0, 256, (3, h, w), dtype=np.uint8)
    want = RB.bayer_to_rgb(frames, pattern)
    if h == 4:                                               # the smallest: an identity camera, every row read
        cam, dist, M, warped = np.eye(3), np.zeros(5), np.diag([64 / w, 48 / h, 1.0]), (64, 48)
    else:                                                    # a bird's-eye view that reads a narrow run of camera rows: rows and rest differ
        q = FM.calibration_sets("A" if w == 64 else "B")[2]
        cam, dist, M, warped = q["cam_matrix"], q["dist_coeffs"], q["M"], (w, h)
    c = _native.Context((w, h), warped, cam, dist, M, capacity=4)
    n = 3
    try:
        c.set_input_format(pattern)
        c.overlay_configure(np.linalg.inv(M))
        c0, c1 = c.source_rows()
        assert h == 4 or (c1 - c0 < h - 8 and c.input_rows() != (c0, c1)), (c0, c1)
        c.upload_frames(frames, first=1)
        assert np.array_equal(_read_back(c, n, h, w, first=1), want), "lt_upload_frames"
        other, exp = np.roll(frames, 1, 0), np.roll(want, 1, 0)                       # rows + rest: the whole frame from two calls
        keep = [c.upload_frame_rows(other, first=1, enqueue=True)]
        c.mask_run(n, first=1)
        keep.append(c.upload_frame_rest(other, first=1))
        assert np.array_equal(_read_back(c, n, h, w, first=1), exp), "rows + rest"
        c.sync()
        third, exp3 = np.roll(frames, 2, 0), np.roll(want, 2, 0)
        runs = (1, 3, 3, 3) if h == 4 else (5, 19, 23, h - 3)                         # odd bounds
        rows = np.array(runs, np.int32)
        keep = [c.upload_frame_rows(third, first=1, enqueue=True)]
        c.mask_run(n, first=1)
        keep.append(c.upload_frame_rest(third, first=1, rows=rows.ctypes.data))
        got = _read_back(c, n, h, w, first=1)
        held = exp.copy()
        for lo, hi in ((runs[0], runs[1]), (runs[2], runs[3])):
            held[:, lo:hi] = exp3[:, lo:hi]
        assert np.array_equal(got, held), ("rows + rest_rows", np.argwhere(got != held)[:4])
        c.sync()
        dev = _surfaces(frames, pattern, pitch=w + 5, offset=3)
        dev2 = _surfaces(other, pattern)                                             # dense and aligned
        try:
            keep = c.attach_device_frames(dev, first=1)
            c.mask_run(n, first=1)
            c.device_frames_rest(n, first=1)
            assert np.array_equal(_read_back(c, n, h, w, first=1), want), "attach + device_frames_rest"
            keep2 = c.attach_device_frames(dev2, first=1)
            c.mask_run(n, first=1)
            c.device_frames_rest(n, first=1, rows=rows.ctypes.data)
            got = _read_back(c, n, h, w, first=1)
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


def test_a_shown_frame_without_a_lane_is_the_demosaiced_frame():
    """process() of a frame in which nothing is found: the annotated frame of a raw Bayer tracker is that of an RGB tracker fed the
    demosaiced frame -- the camera frame as the row conversion wrote it, under whatever both draw."""
    cal = calib.reference_calibration()
    raw = np.random.default_rng(77).integers(0, 256, (H, W), dtype=np.uint8)
    raw[400:] = 0                                            # noise above, a black road: nothing to find
    rgb = RB.bayer_to_rgb(raw, "bayer_gbrg")
    a, b = LaneTracker(**cal, pixel_format="bayer_gbrg"), LaneTracker(**cal)
    try:
        out_a, out_b = a.process(raw), b.process(rgb)
        assert out_a.shape == (H, W, 3) and np.array_equal(out_a, out_b)
        assert b.success == 0 and (out_b[:390] == rgb[:390]).all(-1).mean() > 0.9      # nothing found: the frame is the camera frame itself (but for text)
    finally:
        a.close()
        b.close()


# ---- end to end at the reference calibration --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    """Eight rendered scenes, RGB (shared; never changed)."""
    r = synth.SceneRenderer()
    out = np.stack([r.render(s)[0] for s in range(8)])
    out.setflags(write=False)
    return out


def _state(lt):
    b = lambda a: None if a is None else np.asarray(a).tobytes()
    return dict(detected=lt.detected_pixels, valid=lt.valid_lane_lines, last_detection=lt.last_detection, success=lt.success,
                counter=lt.counter, left_avg=b(lt.left_avg_coeffs), right_avg=b(lt.right_avg_coeffs), last_left=b(lt.last_left_coeffs),
                last_right=b(lt.last_right_coeffs), hist=[b(c) for c in lt.left_fit_coeffs] + [b(c) for c in lt.right_fit_coeffs],
                radii=list(lt.average_curve_radii), radius=lt.average_curve_radius, ecc=lt.eccentricity,
                pix=(b(lt.left_y), b(lt.left_x), b(lt.right_y), b(lt.right_x)), cent=(lt.left_window_centroids, lt.right_window_centroids))


def _pair(pattern):
    cal = calib.reference_calibration()
    return LaneTracker(**cal, pixel_format=pattern), LaneTracker(**cal)


def _states_equal(a, b, pattern):
    sa, sb = a.get_state(), b.get_state()
    assert sa.pop("pixel_format") == pattern
    sa.pop("yuv_matrix")
    assert sa == sb and _state(a) == _state(b)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_trackers_equal_an_rgb_tracker_on_the_demosaiced_frames(pattern, scenes):
    """8 scenes mosaiced by sampling the pattern: process(), process_batch and process_stream of a raw Bayer tracker against an RGB
    tracker fed bayer_to_rgb of the same frames -- annotated frames, masks and records (through the state), get_state()."""
    raw = RB.rgb_to_bayer(scenes, pattern)
    rgb = RB.bayer_to_rgb(raw, pattern)
    a, b = _pair(pattern)
    try:                                                     # process()
        for k in range(8):
            out_b = b.process(rgb[k])
            out_a = a.process(raw[k])
            assert out_a.shape == (H, W, 3) and np.array_equal(out_a, out_b), k
            assert _state(a) == _state(b), k
            assert np.array_equal(a._ctx.download_masks(1), b._ctx.download_masks(1)), k
            assert a._ctx.download_records(1).tobytes() == b._ctx.download_records(1).tobytes(), k
        assert b.get_success_ratio() == (1.0, 8, 8)          # the comparison is not between two failures
        _states_equal(a, b, pattern)
        with pytest.raises(ValueError):
            a.process(rgb[5])
    finally:
        a.close()
        b.close()
    a, b = _pair(pattern)
    try:                                                     # process_batch
        oa, ob = a.process_batch(raw), b.process_batch(rgb)
        assert len(oa) == 8 and all(np.array_equal(x, y) for x, y in zip(oa, ob))
        assert b.get_success_ratio() == (1.0, 8, 8)
        _states_equal(a, b, pattern)
    finally:
        a.close()
        b.close()
    a, b = _pair(pattern)
    try:                                                     # process_stream: windows of 3, 3 and 2
        cut = lambda v: [v[:3], v[3:6], v[6:]]
        for w_, (oa, ob) in enumerate(zip(a.process_stream(cut(raw)), b.process_stream(cut(rgb)))):
            assert len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w_
        assert a.counter == 8 and b.get_success_ratio() == (1.0, 8, 8)
        _states_equal(a, b, pattern)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("fed", ["host", "device"])
def test_group_of_two_cameras_with_their_own_calibrations(fed, scenes):
    from lane_tracker_amd import LaneTrackerGroup
    cams = CC.cameras()
    pattern, k, n = "bayer_bggr", 2, 8
    rgb = [scenes, CC.shifted(scenes)]
    vids = [RB.rgb_to_bayer(v, pattern) for v in rgb]
    conv = [RB.bayer_to_rgb(v, pattern) for v in vids]
    dev = [_surfaces(v, pattern, pitch=W + 5, offset=1) for v in vids] if fed == "device" else None
    g = LaneTrackerGroup(k, **cams["A"], pixel_format=pattern, calibrations=[None, CC.overrides(cams["B"])])
    solos = [LaneTracker(**cams[x]) for x in "AB"]           # RGB trackers, on the demosaiced frames
    try:
        assert g.calibration_count() == 2
        for t in range(n):
            outs = g.process([dev[i][t] if dev else vids[i][t] for i in range(k)])
            for i in range(k):
                want = solos[i].process(conv[i][t])
                assert np.array_equal(outs[i], want), (t, i)
                sg = g.trackers[i].get_state()
                assert sg.pop("pixel_format") == pattern
                sg.pop("yuv_matrix")
                assert sg == solos[i].get_state(), (t, i)
        assert solos[0].get_success_ratio() == (1.0, 8, 8) and solos[1].success > 0
    finally:
        g.close()
        for s in solos:
            s.close()
        for d in dev or ():
            d.owner.close()


@pytest.mark.parametrize("out_layout", ["nv12", "rgb"])
def test_annotated_frames_into_a_sink(out_layout, scenes):
    """out=: a raw Bayer tracker writes the sink an RGB tracker fed the demosaiced frames writes."""
    pattern = "bayer_grbg"
    raw = RB.rgb_to_bayer(scenes[:4], pattern)
    rgb = RB.bayer_to_rgb(raw, pattern)
    a, b = _pair(pattern)
    sa, sb = DeviceFrames.empty(4, (W, H), out_layout, fill=0xEE), DeviceFrames.empty(4, (W, H), out_layout, fill=0xEE)
    try:
        got = a.process_batch(raw, out=sa)
        b.process_batch(rgb, out=sb)
        assert len(got) == 4 and all(isinstance(g, DeviceFrames) and g.pixel_format == out_layout for g in got)
        assert np.array_equal(sa.to_host(), sb.to_host())
        _states_equal(a, b, pattern)
        assert b.success == 4
    finally:
        a.close()
        b.close()
        sa.owner.close()
        sb.owner.close()


# ---- refusals leave the context usable ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_refusals_leave_the_context_usable(pattern):
    w, h = 64, 48
    code = _native.BAYER_FORMATS[pattern]
    k8 = np.array(_native.RGB2YUV_MATRICES["bt601"], np.int32)
    mk = lambda size=(w, h): _native.Context(size, (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=2)
    for size in ((65, 48), (64, 47), (2, 48), (64, 2)):      # odd or too small: LT_ERR_INVALID from the library itself
        odd = mk(size)
        try:
            with pytest.raises(ValueError):
                odd.set_input_format(pattern)
            assert odd.lib.lt_set_input_format(odd._h, code, None) == -1 and b"even width and height" in odd.lib.lt_last_error()
            assert odd.input_format()[0] == "rgb"
        finally:
            odd.close()
    sized = mk()
    try:                                                     # a context with an input size takes RGB only: LT_ERR_STATE
        sized.set_input_size((96, 72))
        assert sized.lib.lt_set_input_format(sized._h, code, None) == -5 and b"input size" in sized.lib.lt_last_error()
        assert sized.input_format()[0] == "rgb"
    finally:
        sized.close()
    fresh = mk()
    try:                                                     # lt_set_input_size on a raw Bayer context: LT_ERR_STATE
        fresh.set_input_format(pattern)
        assert fresh.lib.lt_set_input_size(fresh._h, 96, 72) == -5 and b"RGB" in fresh.lib.lt_last_error()
        assert fresh.input_size() == (w, h) and fresh.input_format()[0] == pattern
    finally:
        fresh.close()
    frames = np.random.default_rng(code).integers(0, 256, (4, h, w), dtype=np.uint8)
    want = RB.bayer_to_rgb(frames, pattern)
    c = mk()
    dev = _surfaces(frames[:2], pattern, pitch=w + 5, offset=1)
    turn = [0]

    def good():
        """Two other frames of the four each time, through the row-run upload: the identity camera's undistorted rows are the frame."""
        turn[0] += 1
        idx = [turn[0] % 4, (turn[0] + 1) % 4]
        c.upload_frame_rows(frames[idx])
        c.mask_run(2)
        r0, r1 = c.info().src_row0, c.info().src_row1
        assert np.array_equal(c.download_undistorted(2), want[idx][:, r0:r1]), turn[0]
    try:
        c.set_input_format(pattern)
        assert c.set_direct_upload(True) == 0                # rows go to staging: the engine takes them
        c.overlay_configure(np.eye(3))
        good()
        c.set_input_format(pattern)                          # the same again is no change
        for other in ("rgb", "nv12", "bgr", PATTERNS[(PATTERNS.index(pattern) + 1) % 4]):
            with pytest.raises(_native.NativeError, match="after its first upload"):      # a format change after an upload
                c.set_input_format(other)
        assert c.input_format()[0] == pattern
        good()
        sink = DeviceFrames.empty(2, (w, h), "rgb")
        try:                                                 # a sink layout of 16 .. 19: LT_ERR_INVALID
            s = np.ascontiguousarray(sink.surfaces)
            assert c.lib.lt_overlay_store_device(c._h, 0, 2, s.ctypes.data, code, k8.ctypes.data) == -1 and b"input format only" in c.lib.lt_last_error()
            src = DeviceBuffer(2 * h * w * 3)
            try:
                assert c.lib.lt_rgb_to_surfaces(0, src.ptr, h * w * 3, h, w, 2, s.ctypes.data, code, k8.ctypes.data) == -1
            finally:
                src.close()
        finally:
            sink.owner.close()
        good()
        ok = np.zeros(2, np.int32)                           # in-place drawing: LT_ERR_STATE before anything is staged
        assert c.lib.lt_overlay_run_inplace(c._h, 0, 2, ok.ctypes.data, ok.ctypes.data, None, None, 0.3, None, k8.ctypes.data) == -5
        assert b"input format only" in c.lib.lt_last_error()
        good()
        assert c.lib.lt_set_input_size(c._h, 96, 72) == -5   # LT_ERR_STATE
        assert c.input_size() == (w, h)
        good()
        short = DeviceFrames(dev.surfaces.copy(), dev.img_size, pattern, owner=dev.owner)
        short.surfaces["pitch"] = w - 1
        with pytest.raises(ValueError, match="pitch"):       # a pitch below W
            c.attach_device_frames(short)
        good()
        past = DeviceFrames(dev.surfaces.copy(), dev.img_size, pattern, owner=dev.owner)
        past.surfaces["plane"][1, 0] += np.uint64(1)         # the block ends on the plane's last byte: one byte further is past it
        with pytest.raises(ValueError, match="past the end"):
            c.attach_device_frames(past)
        good()
        with pytest.raises(ValueError):
            c.upload_frame_rows(np.zeros((2, h, w, 3), np.uint8))
        keep = c.attach_device_frames(dev)                   # ... and the surfaces themselves are taken
        c.mask_run(2)
        r0, r1 = c.info().src_row0, c.info().src_row1
        assert np.array_equal(c.download_undistorted(2), want[:2, r0:r1])
        c.sync()
        del keep
        good()
    finally:
        c.close()
        dev.owner.close()
