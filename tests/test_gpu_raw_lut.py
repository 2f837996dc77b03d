"""Raw tables on the device: the invariant, bit for bit -- whatever a raw Bayer context, tracker or group with table L computes from
frames F is what the same object without a table computes from `utils.apply_raw_lut(F, pattern, L)` -- for the conditioned walk
(k_raw_walk_rows), the conditioned row conversion (k_raw_rows_rgb) and everything behind them.

Sizes A (64 x 48) and B (66 x 50) of front_matrix.py: the smallest that hit both the dword-multiple and the odd row bytes, the
16-column and the byte-wise body of the row conversion.  The tables: four independent random permutations (any phase mix-up shows), the
identity (a set table is never special-cased: the conditioned kernels run) and raw_lut(16, 240, (1.9, 1, 1.6), 'srgb')."""
import numpy as np
import pytest

import bayer_reference as RB
import front_matrix as FM
from lane_tracker_amd import _native, calib, synth, utils
from lane_tracker_amd.device import DeviceBuffer, DeviceFrames, pack_host_frames
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

PATTERNS = list(RB.PATTERNS)
N = 5                                    # slots of a run: ids_pattern(5) = sets 0, 1, 2, 3, 0
CAPACITY = 8
SOURCES = ("upload", "rows", "surfaces")


def permutation_table(seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256) for _ in range(4)]).astype(np.uint8)


def tables():
    return [("permutations", permutation_table(21)), ("identity", utils.raw_lut()), ("srgb", utils.raw_lut(16, 240, (1.9, 1, 1.6), "srgb"))]


def _context(pattern, size, lut=None, capacity=CAPACITY):
    sets = FM.calibration_sets(size)
    c = _native.Context(FM.SIZES[size], FM.SIZES[size], sets[0]["cam_matrix"], sets[0]["dist_coeffs"], sets[0]["M"], capacity=capacity)
    try:
        c.set_input_format(pattern)
        for s, q in enumerate(sets[1:], 1):
            assert c.add_calibration(q["cam_matrix"], q["dist_coeffs"], q["M"]) == s
        c.set_streams(1)
        if lut is not None:
            c.set_raw_lut(lut)
    except BaseException:
        c.close()
        raise
    return c


def _feed(ctx, pattern, size, frames, first, source, offset):
    """The frames into slots first, ... -> what must outlive the run (a DeviceFrames to close, or None)."""
    if source == "upload":
        ctx.upload_frames(frames, first=first)
        return None
    if source == "rows":
        ctx.upload_frames(~frames, first=first)              # what a slot held before is not what is read
        ctx.upload_frame_rows(frames, first=first)
        return None
    ctx.upload_frames(~frames, first=first)                  # the slot's own staging frame is not the one to read
    dev = FM.device_surfaces(frames, pattern, size, offset)  # pitch W + 5, the first plane at byte `offset`
    try:
        ctx.attach_device_frames(dev, first=first)
    except BaseException:
        dev.owner.close()
        raise
    return dev


def _front(ctx, pattern, size, frames, ids, first, source, offset):
    ctx.set_slot_calibrations(ids, first=first)
    dev = _feed(ctx, pattern, size, frames, first, source, offset)
    try:
        ctx.mask_run(len(frames), first=first)
        und = ctx.download_undistorted(len(frames), first=first)
        r, b = ctx.download_plane(0, len(frames), first=first), ctx.download_plane(1, len(frames), first=first)
        ctx.sync()
    finally:
        if dev is not None:
            dev.owner.close()
    return und, r, b


def _oracle_front(size, s, rgb):
    O, oc = FM._oracle(), FM.oracle_calib(size, s)
    bev = O.front_end(oc, rgb)
    return O.undistort(oc, rgb), np.ascontiguousarray(bev[..., 0]), O.lab_b(bev)


@pytest.mark.parametrize("size", ["A", "B"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_front_end_with_a_table_is_the_plain_one_on_the_conditioned_frames(pattern, size):
    """Per table, source and table form (one table: every slot of the run in the same set, each of the four sets in turn; table per
    slot: the mixed id pattern): undistorted rows, R plane and Lab-b plane of a context with table L on F against a context without a
    table on apply_raw_lut(F), and against the oracle on the demosaiced conditioned frames."""
    w, h = FM.SIZES[size]
    pool = FM.frame_pool(pattern, size)
    with_lut, plain = _context(pattern, size, utils.raw_lut()), _context(pattern, size)
    try:
        assert (with_lut.info().src_row0, with_lut.info().src_row1) == (0, h)           # set 0 is the identity: the rows are the whole image
        case = 0
        for name, lut in tables():
            with_lut.set_raw_lut(lut)
            assert np.array_equal(with_lut.raw_lut(), lut) and plain.raw_lut() is None
            for source in SOURCES:
                forms = [("one table, set %d" % s, [s] * N) for s in range(FM.N_SETS)] + [("table per slot", FM.ids_pattern(N))]
                for form, ids in forms:
                    case += 1
                    first, offset = 1 + case % 3, 1 + 2 * (case % 2)                    # odd and even first slots; odd plane offsets
                    frames = pool[[(7 * case + i) % len(pool) for i in range(N)]]
                    cond = utils.apply_raw_lut(frames, pattern, lut)
                    where = "%s %s, table %s, source %s, %s, slots [%d, %d)" % (pattern, size, name, source, form, first, first + N)
                    got = _front(with_lut, pattern, size, frames, ids, first, source, offset)
                    want = _front(plain, pattern, size, cond, ids, first, source, offset)
                    for what, g, p in zip(("undistorted rows", "R plane", "Lab-b plane"), got, want):
                        assert g.shape == p.shape and np.array_equal(g, p), "%s: %d bytes of the %s differ from the plain context's" % (
                            where, int((g != p).sum()), what)
                    rgb = RB.bayer_to_rgb(cond, pattern)
                    for i, s in enumerate(ids):
                        for what, g, o in zip(("undistorted rows", "R plane", "Lab-b plane"), got, _oracle_front(size, s, rgb[i])):
                            assert np.array_equal(g[i], o), "%s: slot %d, set %d: %d bytes of the %s differ from the oracle's" % (
                                where, first + i, s, int((g[i] != o).sum()), what)
    finally:
        with_lut.close()
        plain.close()


# ---- the row conversion ---------------------------------------------------------------------------------------------------------------
def _read_back(c, n, h, w, first):
    """Every row of the camera frames of the slots, through the overlay with no points (a plain copy) over two runs that cover the frame."""
    e = np.zeros(0, np.int64)
    rows = np.array([0, h // 2, h // 2, h], np.int32)
    c.overlay_run([(e, e, e, e)] * n, first=first, rows=rows.ctypes.data)
    out = _native.pinned_empty((n, h, w, 3))
    out[:] = 0
    c.download_overlay_async(out, first=first, rows=rows.ctypes.data)
    c.sync()
    return np.array(out)


def _surfaces(frames, pattern, padded):
    """Dense, 16-byte aligned surfaces, or (padded) five bytes more than a row holds between the rows and the first plane at byte 3."""
    kw = dict(pitch=frames.shape[2] + 5, offset=3) if padded else {}
    block, surf, size, single = pack_host_frames(frames, pattern, fill=FM.FILL, **kw)
    buf = DeviceBuffer(block.nbytes).copy_from_host(block)
    surf["plane"][:, :1] += np.uint64(buf.ptr)
    return DeviceFrames(surf, size, pattern, owner=buf, single=single)


@pytest.mark.parametrize("source", ["slots", "surfaces"])
@pytest.mark.parametrize("size", ["A", "B"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_shown_camera_frame_is_the_demosaic_of_the_conditioned_mosaic(pattern, size, source):
    """The slot's RGB camera frame: whole uploads, then two row runs that include rows 0 and H - 1 (the demosaic's border rule) over the
    frame a former upload left; the 16-column body (W = 64, dense) and the byte-wise one (W = 66; surfaces at pitch W + 5, offset 3)."""
    w, h = FM.SIZES[size]
    n, first = 3, 1
    lut = permutation_table(40 + PATTERNS.index(pattern))
    frames = FM.frame_pool(pattern, size)[10:10 + n]
    fill = np.full_like(frames, FM.FILL)
    show = lambda f: RB.bayer_to_rgb(utils.apply_raw_lut(f, pattern, lut), pattern)
    runs = (0, 3, h - 5, h)
    rows = np.array(runs, np.int32)
    held = show(fill)
    for lo, hi in (runs[:2], runs[2:]):
        held[:, lo:hi] = show(frames)[:, lo:hi]
    q = FM.calibration_sets(size)[0]                         # the identity: every row is read
    c = _native.Context((w, h), (w, h), q["cam_matrix"], q["dist_coeffs"], q["M"], capacity=n + 1)
    try:
        c.set_input_format(pattern)
        c.set_raw_lut(lut)
        c.overlay_configure(np.linalg.inv(q["M"]))
        c.upload_frames(fill, first=first)
        assert np.array_equal(_read_back(c, n, h, w, first), show(fill)), "lt_upload_frames"
        if source == "slots":
            keep = [c.upload_frame_rows(frames, first=first, enqueue=True)]
            c.mask_run(n, first=first)
            keep.append(c.upload_frame_rest(frames, first=first, rows=rows.ctypes.data))
            got = _read_back(c, n, h, w, first)
            del keep
            assert np.array_equal(got, held), ("rows + rest over two runs", np.argwhere(got != held)[:4])
            other = FM.frame_pool(pattern, size)[20:20 + n]
            keep = [c.upload_frame_rows(other, first=first, enqueue=True)]
            c.mask_run(n, first=first)
            keep.append(c.upload_frame_rest(other, first=first))
            got = _read_back(c, n, h, w, first)
            del keep
            assert np.array_equal(got, show(other)), ("rows + rest", np.argwhere(got != show(other))[:4])
        else:
            dev = _surfaces(frames, pattern, padded=size == "B")
            try:
                keep = c.attach_device_frames(dev, first=first)
                c.mask_run(n, first=first)
                c.device_frames_rest(n, first=first, rows=rows.ctypes.data)
                got = _read_back(c, n, h, w, first)
                assert np.array_equal(got, held), ("device_frames_rest over two runs", np.argwhere(got != held)[:4])
                c.device_frames_rest(n, first=first)
                got = _read_back(c, n, h, w, first)
                assert np.array_equal(got, show(frames)), ("device_frames_rest", np.argwhere(got != show(frames))[:4])
                del keep
            finally:
                dev.owner.close()
    finally:
        c.close()


# ---- switching tables -----------------------------------------------------------------------------------------------------------------
def test_switching_tables_over_reused_slots():
    """Table 1, then table 2, then none over the same slots and the same staged frames: each run is right (a front end is not reused
    across the call, lt_mask_rerun included), lt_get_raw_lut round-trips, and the table belongs to raw Bayer input."""
    pattern, size = "bayer_grbg", "A"
    one, two = permutation_table(61), utils.raw_lut(16, 240, (1.9, 1, 1.6), "srgb")
    frames = FM.frame_pool(pattern, size)[30:30 + N]
    ids = [2] * N
    c, plain = _context(pattern, size), _context(pattern, size)
    try:
        assert c.raw_lut() is None
        c.set_slot_calibrations(ids, first=1)
        c.upload_frames(frames, first=1)
        for step, lut in enumerate((one, two, None, one)):
            c.set_raw_lut(lut)
            got_lut = c.raw_lut()
            assert (got_lut is None) if lut is None else np.array_equal(got_lut, lut)
            c.mask_run(N, first=1, reuse_front=step == 3)                               # the frames stay staged: only the table changed
            got = (c.download_undistorted(N, first=1), c.download_plane(0, N, first=1), c.download_plane(1, N, first=1))
            cond = frames if lut is None else utils.apply_raw_lut(frames, pattern, lut)
            want = _front(plain, pattern, size, cond, ids, 1, "upload", 0)
            for g, p in zip(got, want):
                assert np.array_equal(g, p), (step, int((g != p).sum()))
    finally:
        c.close()
        plain.close()
    q = FM.calibration_sets(size)[0]
    rgb = _native.Context(FM.SIZES[size], FM.SIZES[size], q["cam_matrix"], q["dist_coeffs"], q["M"], capacity=1)
    try:
        assert rgb.lib.lt_set_raw_lut(rgb._h, one.ctypes.data) == -5 and b"raw Bayer" in rgb.lib.lt_last_error()      # LT_ERR_STATE
        assert rgb.lib.lt_set_raw_lut(rgb._h, None) == -5
        assert rgb.raw_lut() is None
        rgb.set_input_format(pattern)
        rgb.set_raw_lut(one)
        assert np.array_equal(rgb.raw_lut(), one)
        rgb.set_input_format("rgb")                              # a layout that is not raw Bayer removes the table
        rgb.set_input_format(pattern)
        assert rgb.raw_lut() is None
    finally:
        rgb.close()


# ---- trackers and groups at the reference calibration ---------------------------------------------------------------------------------
def _state(lt):
    b = lambda a: None if a is None else np.asarray(a).tobytes()
    return dict(detected=lt.detected_pixels, valid=lt.valid_lane_lines, last_detection=lt.last_detection, success=lt.success,
                counter=lt.counter, left_avg=b(lt.left_avg_coeffs), right_avg=b(lt.right_avg_coeffs), last_left=b(lt.last_left_coeffs),
                last_right=b(lt.last_right_coeffs), hist=[b(c) for c in lt.left_fit_coeffs] + [b(c) for c in lt.right_fit_coeffs],
                radii=list(lt.average_curve_radii), radius=lt.average_curve_radius, ecc=lt.eccentricity,
                pix=(b(lt.left_y), b(lt.left_x), b(lt.right_y), b(lt.right_x)), cent=(lt.left_window_centroids, lt.right_window_centroids))


def _same(a, b):
    assert a.get_state() == b.get_state() and _state(a) == _state(b)


def test_trackers_and_a_group_equal_plain_ones_on_the_conditioned_frames():
    """Six rendered scenes, mosaiced and put onto a sensor's pedestal at half scale; the table undoes that and balances the colours.
    process(), process_batch (annotated), process_stream over frames in device memory and a group of two: annotated frames, records
    and get_state() are those of plain raw Bayer trackers fed the conditioned frames."""
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    pattern = "bayer_gbrg"
    r = synth.SceneRenderer()
    raw = (RB.rgb_to_bayer(np.stack([r.render(s)[0] for s in range(6)]), pattern) // 2 + 16).astype(np.uint8)
    lut = utils.raw_lut(16, 143, (1.05, 1, 0.95), 1.1)
    cond = utils.apply_raw_lut(raw, pattern, lut)
    pair = lambda: (LaneTracker(**cal, pixel_format=pattern, raw_lut=lut), LaneTracker(**cal, pixel_format=pattern))
    a, b = pair()
    try:                                                     # process()
        for k in range(3):
            oa, ob = a.process(raw[k]), b.process(cond[k])
            assert oa.shape == (H, W, 3) and np.array_equal(oa, ob), k
            assert a._ctx.download_records(1).tobytes() == b._ctx.download_records(1).tobytes(), k
            assert np.array_equal(a._ctx.download_masks(1), b._ctx.download_masks(1)), k
        _same(a, b)
        assert b.success == 3                                # the comparison is not between two failures
    finally:
        a.close()
        b.close()
    a, b = pair()
    try:                                                     # process_batch, annotated
        oa, ob = a.process_batch(raw), b.process_batch(cond)
        assert len(oa) == 6 and all(np.array_equal(x, y) for x, y in zip(oa, ob))
        _same(a, b)
        assert b.get_success_ratio() == (1.0, 6, 6)
    finally:
        a.close()
        b.close()
    dev_raw, dev_cond = _surfaces(raw, pattern, padded=True), _surfaces(cond, pattern, padded=True)
    a, b = pair()
    try:                                                     # process_stream over DeviceFrames: windows of 3, 2 and 1
        cut = lambda v: [v[:3], v[3:5], v[5:]]
        for w_, (oa, ob) in enumerate(zip(a.process_stream(cut(dev_raw)), b.process_stream(cut(dev_cond)))):
            assert len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w_
        assert a.counter == 6
        _same(a, b)
    finally:
        a.close()
        b.close()
        dev_raw.owner.close()
        dev_cond.owner.close()
    g, solos = LaneTrackerGroup(2, **cal, pixel_format=pattern, raw_lut=lut), [LaneTracker(**cal, pixel_format=pattern) for _ in range(2)]
    try:                                                     # a group of two: stream 1 runs two frames ahead
        for t in range(4):
            outs = g.process([raw[t], raw[t + 2]])
            for i, k in enumerate((t, t + 2)):
                assert np.array_equal(outs[i], solos[i].process(cond[k])), (t, i)
                assert g.trackers[i].get_state() == solos[i].get_state(), (t, i)
        assert solos[0].success == 4
    finally:
        g.close()
        for s in solos:
            s.close()
