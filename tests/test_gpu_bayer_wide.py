"""10- / 12-bit raw Bayer on the device: the invariant, bit for bit -- whatever a context, tracker or group in 'bayerNN_P' with table L
computes from uint16 frames F is what the 8-bit 'bayer_P' object without a table computes from `utils.apply_raw_lut(F, 'bayerNN_P', L)`
-- for the wide walk (k_raw_walk_rows, STAGES bit 0), the wide row conversion (k_raw_rows_rgb, the same bit) and everything behind them.

Sizes A (64 x 48) and B (66 x 50) of front_matrix.py: the smallest that hit both the dword-multiple and the odd row bytes, the
16-column and the site-wise body of the row conversion.  Frames: the 8-bit pool's mosaics shifted up by bits - 8 with random low bits,
plus an all-zero frame, an all-maximum frame and a frame with random bits set above the sample (they are ignored).  Tables: a random
(4, 2**bits) table with independently drawn rows (any phase mix-up shows), the default, and raw_lut(64, 3840, (1.9, 1, 1.6), 'srgb',
bits=12) with its 10-bit counterpart.  Wide surfaces: pitch 2 W + 6, the plane at byte 2 of its block."""
import functools

import numpy as np
import pytest

import bayer_reference as RB
import front_matrix as FM
from lane_tracker_amd import _native, calib, synth, utils
from lane_tracker_amd.device import DeviceBuffer, DeviceFrames, pack_host_frames
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

PATTERNS = list(RB.PATTERNS)             # the 8-bit names, in pattern order
DEPTHS = (10, 12)
N = 5                                    # slots of a run: ids_pattern(5) = sets 0, 1, 2, 3, 0
CAPACITY = 8
SOURCES = ("upload", "rows", "surfaces")
POOL = 24


def wide_name(pattern, bits):
    return "bayer%d_%s" % (bits, pattern[6:])


@functools.lru_cache(maxsize=None)
def tables(bits):
    scale = 1 << (bits - 10)
    out = [("random", np.random.default_rng(21 + bits).integers(0, 256, (4, 1 << bits), dtype=np.uint8)), ("default", utils.raw_lut(bits=bits)),
           ("srgb", utils.raw_lut(16 * scale, 960 * scale, (1.9, 1, 1.6), "srgb", bits=bits))]
    for _, t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wide_pool(pattern, bits, size):
    """POOL frames: frames 0, 1, 2 the all-zero one, the all-maximum one and one with random bits above the sample."""
    rng = np.random.default_rng(FM.case_seed(pattern, size) + bits)
    m = FM.frame_pool(pattern, size)[:POOL].astype(np.uint16)
    out = (m << (bits - 8)) | rng.integers(0, 1 << (bits - 8), m.shape, dtype=np.uint16)
    out[0] = 0
    out[1] = (1 << bits) - 1
    out[2] |= rng.integers(1, 1 << (16 - bits), m.shape[1:], dtype=np.uint16) << bits
    assert out.dtype == np.uint16 and (out[3:] >> bits == 0).all() and (out[2] >> bits).all()
    out.setflags(write=False)
    return out


def _context(fmt, size, lut=None, capacity=CAPACITY):
    sets = FM.calibration_sets(size)
    c = _native.Context(FM.SIZES[size], FM.SIZES[size], sets[0]["cam_matrix"], sets[0]["dist_coeffs"], sets[0]["M"], capacity=capacity)
    try:
        c.set_input_format(fmt)
        for s, q in enumerate(sets[1:], 1):
            assert c.add_calibration(q["cam_matrix"], q["dist_coeffs"], q["M"]) == s
        c.set_streams(1)
        if lut is not None:
            c.set_raw_lut(lut)
    except BaseException:
        c.close()
        raise
    return c


def _wide_surfaces(frames, fmt, padded=True):
    """Pitch 2 W + 6 and the first plane at byte 2 of the block; or (not padded) dense from the block's first byte."""
    kw = dict(pitch=2 * frames.shape[-1] + 6, offset=2) if padded else {}
    block, surf, size, single = pack_host_frames(frames, fmt, fill=FM.FILL, **kw)
    buf = DeviceBuffer(block.nbytes).copy_from_host(block)
    surf["plane"][:, :1] += np.uint64(buf.ptr)
    return DeviceFrames(surf, size, fmt, owner=buf, single=single)


def _narrow_surfaces(frames, pattern, padded=True):
    kw = dict(pitch=frames.shape[-1] + 5, offset=3) if padded else {}
    block, surf, size, single = pack_host_frames(frames, pattern, fill=FM.FILL, **kw)
    buf = DeviceBuffer(block.nbytes).copy_from_host(block)
    surf["plane"][:, :1] += np.uint64(buf.ptr)
    return DeviceFrames(surf, size, pattern, owner=buf, single=single)


def _surfaces_of(frames, fmt):
    return _wide_surfaces(frames, fmt) if fmt in _native.BAYER_WIDE_FORMATS else _narrow_surfaces(frames, fmt)


def _front(ctx, fmt, frames, ids, first, source):
    ctx.set_slot_calibrations(ids, first=first)
    dev = None
    if source == "upload":
        ctx.upload_frames(frames, first=first)
    elif source == "rows":
        ctx.upload_frames(~frames, first=first)              # what a slot held before is not what is read
        ctx.upload_frame_rows(frames, first=first)
    else:
        ctx.upload_frames(~frames, first=first)              # the slot's own staging frame is not the one to read
        dev = _surfaces_of(frames, fmt)
    try:
        if dev is not None:
            ctx.attach_device_frames(dev, first=first)
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


# ---- 1. the front end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["A", "B"])
@pytest.mark.parametrize("bits", DEPTHS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_wide_front_end_is_the_8_bit_one_on_the_conditioned_frames(pattern, bits, size):
    """Per source and table form (one table: every slot of the run in the same set, each of the four sets in turn; table per slot: the
    mixed id pattern at an odd and at an even first slot), the tables taken in turn: undistorted rows, R plane and Lab-b plane of a wide
    context with table L on F against an 8-bit context without a table on apply_raw_lut(F), and against the oracle on the demosaiced
    conditioned frames."""
    w, h = FM.SIZES[size]
    fmt, pool = wide_name(pattern, bits), wide_pool(pattern, bits, size)
    wide, plain = _context(fmt, size), _context(pattern, size)
    try:
        assert (wide.info().src_row0, wide.info().src_row1) == (0, h)                      # set 0 is the identity: the rows are the whole image
        assert np.array_equal(wide.raw_lut(), utils.raw_lut(bits=bits)) and plain.raw_lut() is None      # installed with the format
        case = 0
        for source in SOURCES:
            forms = [("one table, set %d" % s, [s] * N, None) for s in range(FM.N_SETS)] + \
                    [("table per slot", FM.ids_pattern(N), 1), ("table per slot", FM.ids_pattern(N), 2)]
            for form, ids, at in forms:
                name, lut = tables(bits)[case % 3]
                first = at if at is not None else 1 + case % 3
                frames = pool[[(7 * case + i) % POOL for i in range(N)]]                     # (case 0: the three special frames)
                case += 1
                wide.set_raw_lut(lut)
                assert np.array_equal(wide.raw_lut(), lut)
                cond = utils.apply_raw_lut(frames, fmt, lut)
                where = "%s %s, table %s, source %s, %s, slots [%d, %d)" % (fmt, size, name, source, form, first, first + N)
                got = _front(wide, fmt, frames, ids, first, source)
                want = _front(plain, pattern, cond, ids, first, source)
                for what, g, p in zip(("undistorted rows", "R plane", "Lab-b plane"), got, want):
                    assert g.shape == p.shape and np.array_equal(g, p), "%s: %d bytes of the %s differ from the 8-bit context's" % (
                        where, int((g != p).sum()), what)
                rgb = RB.bayer_to_rgb(cond, pattern)
                for i, s in enumerate(ids):
                    for what, g, o in zip(("undistorted rows", "R plane", "Lab-b plane"), got, _oracle_front(size, s, rgb[i])):
                        assert np.array_equal(g[i], o), "%s: slot %d, set %d: %d bytes of the %s differ from the oracle's" % (
                            where, first + i, s, int((g[i] != o).sum()), what)
        wide.set_raw_lut(None)                                                             # back to the default
        assert np.array_equal(wide.raw_lut(), utils.raw_lut(bits=bits))
    finally:
        wide.close()
        plain.close()


# ---- 2. the row conversion ----------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("size", ["A", "B"])
@pytest.mark.parametrize("bits", DEPTHS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_shown_camera_frame_is_the_8_bit_contexts(pattern, bits, size):
    """The slot's RGB camera frame of a wide context against the 8-bit context's on the conditioned frames and against NumPy: whole
    uploads, row runs that include rows 0 and H - 1 (the demosaic's border rule) over what a former upload left, and attached surfaces;
    the 16-column body (W = 64, dense) and the site-wise one (W = 66; surfaces at pitch 2 W + 6, the plane at byte 2)."""
    w, h = FM.SIZES[size]
    n, first = 3, 1
    fmt = wide_name(pattern, bits)
    lut = tables(bits)[0][1]
    frames, fill = wide_pool(pattern, bits, size)[:n], np.full((n, h, w), 0xEEEE, np.uint16)
    cond = lambda f: utils.apply_raw_lut(f, fmt, lut)
    show = lambda f: RB.bayer_to_rgb(cond(f), pattern)
    runs = (0, 3, h - 5, h)
    rows = np.array(runs, np.int32)
    held = show(fill)
    for lo, hi in (runs[:2], runs[2:]):
        held[:, lo:hi] = show(frames)[:, lo:hi]
    q = FM.calibration_sets(size)[0]                         # the identity: every row is read
    mk = lambda: _native.Context((w, h), (w, h), q["cam_matrix"], q["dist_coeffs"], q["M"], capacity=n + 1)
    c, p = mk(), mk()
    try:
        c.set_input_format(fmt)
        c.set_raw_lut(lut)
        p.set_input_format(pattern)
        for x in (c, p):
            x.overlay_configure(np.linalg.inv(q["M"]))
        c.upload_frames(fill, first=first)
        p.upload_frames(cond(fill), first=first)
        got, ref = _read_back(c, n, h, w, first), _read_back(p, n, h, w, first)
        assert np.array_equal(got, ref) and np.array_equal(got, show(fill)), "lt_upload_frames"
        keep = [c.upload_frame_rows(frames, first=first, enqueue=True), p.upload_frame_rows(cond(frames), first=first, enqueue=True)]
        c.mask_run(n, first=first)
        p.mask_run(n, first=first)
        keep += [c.upload_frame_rest(frames, first=first, rows=rows.ctypes.data), p.upload_frame_rest(cond(frames), first=first, rows=rows.ctypes.data)]
        got, ref = _read_back(c, n, h, w, first), _read_back(p, n, h, w, first)
        del keep
        assert np.array_equal(got, ref) and np.array_equal(got, held), ("rows + rest over two runs", np.argwhere(got != held)[:4])
        other = wide_pool(pattern, bits, size)[10:10 + n]
        dev, dev8 = _wide_surfaces(other, fmt, padded=size == "B"), _narrow_surfaces(cond(other), pattern, padded=size == "B")
        try:
            keep = [c.attach_device_frames(dev, first=first), p.attach_device_frames(dev8, first=first)]
            c.mask_run(n, first=first)
            p.mask_run(n, first=first)
            c.device_frames_rest(n, first=first)
            p.device_frames_rest(n, first=first)
            got, ref = _read_back(c, n, h, w, first), _read_back(p, n, h, w, first)
            del keep
            assert np.array_equal(got, ref) and np.array_equal(got, show(other)), ("device_frames_rest", np.argwhere(got != show(other))[:4])
        finally:
            dev.owner.close()
            dev8.owner.close()
    finally:
        c.close()
        p.close()


@pytest.mark.parametrize("bits", DEPTHS)
def test_bayer_to_rgb_of_wide_frames_is_the_numpy_reference(bits):
    for p, pattern in enumerate(PATTERNS):
        fmt = wide_name(pattern, bits)
        for size in ("A", "B"):
            frames = wide_pool(pattern, bits, size)[:4]
            name, lut = tables(bits)[(p + "AB".index(size)) % 3]
            got = utils.bayer_to_rgb(frames, fmt, raw_lut=lut)
            assert got.shape == frames.shape + (3,) and np.array_equal(got, RB.bayer_to_rgb(utils.apply_raw_lut(frames, fmt, lut), pattern)), (fmt, size, name)
            one = utils.bayer_to_rgb(frames[3], fmt)                                           # no table: the default
            assert np.array_equal(one, RB.bayer_to_rgb(utils.apply_raw_lut(frames[3], fmt, utils.raw_lut(bits=bits)), pattern)), (fmt, size)
        with pytest.raises(ValueError):
            utils.bayer_to_rgb(frames.astype(np.uint8), fmt)
        with pytest.raises(ValueError):
            utils.bayer_to_rgb(frames, fmt, raw_lut=tables(22 - bits)[0][1])
        with pytest.raises(ValueError):
            utils.bayer_to_rgb(frames, pattern)                                               # uint16 frames, an 8-bit pattern


# ---- 3. trackers and groups at the reference calibration ----------------------------------------------------------------------------------
def _state(lt):
    b = lambda a: None if a is None else np.asarray(a).tobytes()
    return dict(detected=lt.detected_pixels, valid=lt.valid_lane_lines, last_detection=lt.last_detection, success=lt.success,
                counter=lt.counter, left_avg=b(lt.left_avg_coeffs), right_avg=b(lt.right_avg_coeffs), last_left=b(lt.last_left_coeffs),
                last_right=b(lt.last_right_coeffs), hist=[b(c) for c in lt.left_fit_coeffs] + [b(c) for c in lt.right_fit_coeffs],
                radii=list(lt.average_curve_radii), radius=lt.average_curve_radius, ecc=lt.eccentricity,
                pix=(b(lt.left_y), b(lt.left_x), b(lt.right_y), b(lt.right_x)), cent=(lt.left_window_centroids, lt.right_window_centroids))


def _get_state(t):
    s = t.get_state()
    assert s.pop("pixel_format") == t.pixel_format and "raw_lut" not in s
    return s


def _same(a, b):
    assert _get_state(a) == _get_state(b) and _state(a) == _state(b)


@functools.lru_cache(maxsize=None)
def _scenes(pattern, bits):
    """Six rendered scenes, mosaiced and put onto a sensor's pedestal (a sixteenth of full scale) below three quarters of full scale,
    noise in the low bits -> (the frames, the table that undoes it and balances the colours, a second table)."""
    r = synth.SceneRenderer()
    m = RB.rgb_to_bayer(np.stack([r.render(s)[0] for s in range(6)]), pattern).astype(np.uint16)
    k, top = 1 << (bits - 9), 1 << bits                      # half scale
    raw = m * k + top // 16 + np.random.default_rng(bits).integers(0, k, m.shape, dtype=np.uint16)
    one = utils.raw_lut(top // 16, top // 16 + 255 * k, (1.05, 1, 0.95), 1.1, bits=bits)
    two = utils.raw_lut(top // 16, top // 16 + 255 * k, (1, 1, 1.02), 1.0, bits=bits)
    raw.setflags(write=False)
    return raw, one, two


@pytest.mark.parametrize("pattern,bits", [("bayer_gbrg", 12), ("bayer_grbg", 10)])
def test_process_and_process_batch_equal_the_8_bit_trackers(pattern, bits):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    fmt = wide_name(pattern, bits)
    raw, lut, _ = _scenes(pattern, bits)
    cond = utils.apply_raw_lut(raw, fmt, lut)
    pair = lambda: (LaneTracker(**cal, pixel_format=fmt, raw_lut=lut), LaneTracker(**cal, pixel_format=pattern))
    a, b = pair()
    try:                                                     # process()
        for k in range(3):
            oa, ob = a.process(raw[k]), b.process(cond[k])
            assert oa.shape == (H, W, 3) and np.array_equal(oa, ob), k
            assert a._ctx.download_records(1).tobytes() == b._ctx.download_records(1).tobytes(), k
            assert np.array_equal(a._ctx.download_masks(1), b._ctx.download_masks(1)), k
        _same(a, b)
        assert b.success == 3                                # the comparison is not between two failures
        with pytest.raises(ValueError, match="uint"):
            a.process(cond[0])                               # uint8 frames are refused, not cast
        with pytest.raises(ValueError, match="uint"):
            b.process(raw[0])
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


@pytest.mark.parametrize("pattern,bits", [("bayer_rggb", 12), ("bayer_bggr", 10)])
def test_process_stream_over_device_frames_with_a_table_change_between_windows(pattern, bits):
    cal = calib.reference_calibration()
    fmt = wide_name(pattern, bits)
    raw, one, two = _scenes(pattern, bits)
    cond = np.concatenate([utils.apply_raw_lut(raw[:3], fmt, one), utils.apply_raw_lut(raw[3:], fmt, two)])
    dev_raw, dev_cond = _wide_surfaces(raw, fmt), _narrow_surfaces(cond, pattern)
    a, b = LaneTracker(**cal, pixel_format=fmt, raw_lut=one), LaneTracker(**cal, pixel_format=pattern)
    try:
        for w_, (oa, ob) in enumerate(zip(a.process_stream([dev_raw[:2], dev_raw[2:3]]), b.process_stream([dev_cond[:2], dev_cond[2:3]]))):
            assert len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w_
        _same(a, b)
        a.set_raw_lut(two)                                   # between windows: an auto-white-balance step
        assert np.array_equal(a.raw_lut, two) and np.array_equal(a._ctx.raw_lut(), two)
        for w_, (oa, ob) in enumerate(zip(a.process_stream([raw[3:5], raw[5:]]), b.process_stream([cond[3:5], cond[5:]]))):     # host frames this time
            assert len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w_
        assert a.counter == 6 and b.success >= 5
        _same(a, b)
        with pytest.raises(ValueError, match="input format only"):
            a.process_batch(dev_raw[:2], out="inplace")
    finally:
        a.close()
        b.close()
        dev_raw.owner.close()
        dev_cond.owner.close()


@pytest.mark.parametrize("pattern,bits", [("bayer_grbg", 12), ("bayer_gbrg", 10)])
def test_a_group_and_a_sink_equal_the_8_bit_ones(pattern, bits):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    fmt = wide_name(pattern, bits)
    raw, lut, _ = _scenes(pattern, bits)
    cond = utils.apply_raw_lut(raw, fmt, lut)
    g, solos = LaneTrackerGroup(2, **cal, pixel_format=fmt, raw_lut=lut), [LaneTracker(**cal, pixel_format=pattern) for _ in range(2)]
    dev = _wide_surfaces(raw, fmt)
    try:                                                     # a group of two: stream 1 runs two frames ahead, and takes device frames
        assert np.array_equal(g.raw_lut, lut) and np.array_equal(g._ctx.raw_lut(), lut)
        for t in range(4):
            outs = g.process([raw[t], dev[t + 2]])
            for i, k in enumerate((t, t + 2)):
                assert np.array_equal(outs[i], solos[i].process(cond[k])), (t, i)
                assert _get_state(g.trackers[i]) == _get_state(solos[i]), (t, i)
        assert solos[0].success == 4
    finally:
        g.close()
        dev.owner.close()
        for s in solos:
            s.close()
    a, b = LaneTracker(**cal, pixel_format=fmt, raw_lut=lut), LaneTracker(**cal, pixel_format=pattern)
    sa, sb = DeviceFrames.empty(4, (W, H), "nv12", fill=0xEE), DeviceFrames.empty(4, (W, H), "nv12", fill=0xEE)
    try:                                                     # out=: annotated frames into an NV12 sink
        got = a.process_batch(raw[:4], out=sa)
        b.process_batch(cond[:4], out=sb)
        assert len(got) == 4 and all(isinstance(x, DeviceFrames) and x.pixel_format == "nv12" for x in got)
        assert np.array_equal(sa.to_host(), sb.to_host())
        _same(a, b)
        assert b.success == 4
        with pytest.raises(ValueError, match="input format only"):
            a.process_batch(raw[:2], out=DeviceFrames(sa.surfaces[:2], (W, H), fmt))     # a wide format as a sink
    finally:
        a.close()
        b.close()
        sa.owner.close()
        sb.owner.close()


# ---- 4. refusals from the library itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", DEPTHS)
def test_the_library_refuses(bits):
    w, h = 64, 48
    fmt = "bayer%d_grbg" % bits
    code, n = _native.BAYER_WIDE_FORMATS[fmt], 1 << bits
    k8 = np.array(_native.RGB2YUV_MATRICES["bt601"], np.int32)
    mk = lambda size=(w, h): _native.Context(size, (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=2)
    for size in ((65, 48), (64, 47), (2, 48), (64, 2)):      # odd or too small: LT_ERR_INVALID from the library itself
        odd = mk(size)
        try:
            with pytest.raises(ValueError):
                odd.set_input_format(fmt)
            assert odd.lib.lt_set_input_format(odd._h, code, None) == -1 and b"even width and height" in odd.lib.lt_last_error()
            assert odd.input_format()[0] == "rgb"
        finally:
            odd.close()
    sized = mk()
    try:                                                     # a context with an input size takes RGB only: LT_ERR_STATE
        sized.set_input_size((96, 72))
        assert sized.lib.lt_set_input_format(sized._h, code, None) == -5 and b"input size" in sized.lib.lt_last_error()
        assert sized.lib.lt_set_input_format(sized._h, code + 4, None) == -1 and sized.lib.lt_set_input_format(sized._h, 8, None) == -1     # no such layouts
        assert sized.input_format()[0] == "rgb"
    finally:
        sized.close()
    table, small = np.random.default_rng(bits).integers(0, 256, (4, n), dtype=np.uint8), utils.raw_lut()
    frames = np.random.default_rng(code).integers(0, 1 << 16, (2, h, w), dtype=np.uint16)
    want = RB.bayer_to_rgb(utils.apply_raw_lut(frames, fmt, table), "bayer_grbg")
    c, narrow = mk(), mk()
    dev = _wide_surfaces(frames, fmt)

    def good():
        """The identity camera's undistorted rows are the demosaic of the conditioned frame: the context still works."""
        c.upload_frame_rows(frames)
        c.mask_run(2)
        r0, r1 = c.info().src_row0, c.info().src_row1
        assert np.array_equal(c.download_undistorted(2), want[:, r0:r1])
    try:
        c.set_input_format(fmt)
        narrow.set_input_format("bayer_grbg")
        assert c.set_direct_upload(True) == 0                # rows go to staging: the engine takes them
        c.set_raw_lut(table)
        c.overlay_configure(np.eye(3))
        good()
        out = np.zeros((4, n), np.uint8)
        for entries in (256, n // 2, n * 2, 22 - bits, 0):   # a wrong `entries`: LT_ERR_INVALID
            assert c.lib.lt_set_raw_lut_wide(c._h, table.ctypes.data, entries) == -1 and b"entries" in c.lib.lt_last_error()
            assert c.lib.lt_get_raw_lut_wide(c._h, out.ctypes.data, entries) == -1
        assert not out.any() and np.array_equal(c.raw_lut(), table)
        assert c.lib.lt_set_raw_lut(c._h, small.ctypes.data) == -5 and c.lib.lt_set_raw_lut(c._h, None) == -5      # the 8-bit call on a wide context
        assert narrow.lib.lt_set_raw_lut_wide(narrow._h, table.ctypes.data, n) == -5                               # ... and the reverse: LT_ERR_STATE
        assert narrow.lib.lt_get_raw_lut_wide(narrow._h, out.ctypes.data, n) == -5 and narrow.raw_lut() is None
        good()
        for field, delta in (("pitch", 1), ("plane", 1), ("pitch", -8)):      # an odd pitch, an odd address, a pitch below the row
            bad = DeviceFrames(dev.surfaces.copy(), dev.img_size, fmt, owner=dev.owner)
            if field == "pitch":
                bad.surfaces["pitch"] += delta
            else:
                bad.surfaces["plane"][:, 0] += np.uint64(delta)
            s = np.ascontiguousarray(bad.surfaces)
            assert c.lib.lt_attach_device_frames(c._h, s.ctypes.data, 0, 2) == -1, (field, delta)
            assert (b"even" if delta == 1 else b"pitch") in c.lib.lt_last_error()
        good()
        sink = DeviceFrames.empty(2, (w, h), "rgb")
        try:                                                 # a wide layout as a sink: LT_ERR_INVALID
            s = np.ascontiguousarray(sink.surfaces)
            assert c.lib.lt_overlay_store_device(c._h, 0, 2, s.ctypes.data, code, k8.ctypes.data) == -1 and b"input format only" in c.lib.lt_last_error()
            src = DeviceBuffer(2 * h * w * 3)
            try:
                assert c.lib.lt_rgb_to_surfaces(0, src.ptr, h * w * 3, h, w, 2, s.ctypes.data, code, k8.ctypes.data) == -1
            finally:
                src.close()
        finally:
            sink.owner.close()
        c.attach_device_frames(dev)
        ok = np.zeros(2, np.int32)                           # in-place drawing: LT_ERR_STATE
        assert c.lib.lt_overlay_run_inplace(c._h, 0, 2, ok.ctypes.data, ok.ctypes.data, None, None, 0.3, None, k8.ctypes.data) == -5
        assert b"input format only" in c.lib.lt_last_error()
        assert c.lib.lt_set_input_size(c._h, 96, 72) == -5   # LT_ERR_STATE
        c.mask_run(2)
        r0, r1 = c.info().src_row0, c.info().src_row1
        assert np.array_equal(c.download_undistorted(2), want[:, r0:r1])       # the attached surfaces, after all of that
        o = np.zeros((h, w, 3), np.uint8)
        assert c.lib.lt_raw16_to_rgb(c._h, frames.ctypes.data, h, w, 16, table.ctypes.data, o.ctypes.data) == -1      # an 8-bit layout
        assert c.lib.lt_raw16_to_rgb(c._h, frames.ctypes.data, h + 1, w, code, table.ctypes.data, o.ctypes.data) == -1
        assert c.lib.lt_bayer_to_rgb(c._h, frames.ctypes.data, h, w, code, o.ctypes.data) == -1
        assert not o.any()
    finally:
        c.close()
        narrow.close()
        dev.owner.close()


# ---- 5. memory -----------------------------------------------------------------------------------------------------------------------------
def test_wide_contexts_and_trackers_give_their_memory_back():
    """Create, use and close a wide context and a wide tracker: the device cache's live bytes are what they were (the table's block
    is freed with the context)."""
    cal = calib.reference_calibration()
    fmt, size = "bayer12_bggr", "A"
    raw, lut, _ = _scenes("bayer_bggr", 12)
    live = lambda: _native.device_cache_stats()["live_bytes"]
    base = live()
    c = _context(fmt, size, tables(12)[0][1])
    try:
        assert live() > base
        _front(c, fmt, wide_pool("bayer_bggr", 12, size)[:N], [0] * N, 1, "surfaces")
    finally:
        c.close()
    assert live() == base
    t = LaneTracker(**cal, pixel_format=fmt, raw_lut=lut)
    try:
        t.process_batch(raw[:3])
        t.set_raw_lut(None)
        t.process(raw[3])
    finally:
        t.close()
    assert live() == base
