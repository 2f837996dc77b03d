"""The colour stage of raw Bayer input on the device: the invariant, bit for bit -- whatever a raw Bayer context, tracker or group with
stage (M, T) and, if set, raw table L computes from frames F is what an RGB one computes from
`utils.apply_raw_color(bayer_to_rgb(apply_raw_lut(F, pattern, L), pattern), M, T)`, the frames converted on the host -- for the walks
(k_raw_walk_rows with STAGES 2 and 3), the row conversions (k_raw_rows_rgb, the same) and everything behind them.

Sizes A (64 x 48) and B (66 x 50) of front_matrix.py: the smallest that hit both the dword-multiple and the odd row bytes, the
16-column and the any-width body of the row conversion.  Frames: the pools of test_gpu_bayer.py (front_matrix.frame_pool) and of
test_gpu_bayer_wide.py (wide_pool).  Stages: the identity, a channel permutation, a random full-range int16 matrix with a random curve,
and a camera's matrix with the sRGB curve."""
import functools

import numpy as np
import pytest

import bayer_reference as RB
import front_matrix as FM
import test_gpu_bayer_wide as BW
from lane_tracker_amd import _native, calib, synth, utils
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

PATTERNS = list(RB.PATTERNS)
N = BW.N                                 # slots of a run: ids_pattern(5) = sets 0, 1, 2, 3, 0
SOURCES = ("upload", "rows", "surfaces")
KINDS = ("8", "8lut", "10", "12")        # 8-bit without a table, 8-bit behind a random table, 10 bits, 12 bits
IDENT_M = (np.eye(3) * 1024).astype(np.int16)
IDENT_T = np.arange(256, dtype=np.uint8)
CAMERA = [[1.9, -0.7, -0.2], [-0.3, 1.6, -0.3], [0.0, -0.6, 1.6]]


@functools.lru_cache(maxsize=None)
def stages():
    rng = np.random.default_rng(77)
    out = [("identity", IDENT_M, IDENT_T),
           ("permutation", np.array([[0, 1024, 0], [0, 0, 1024], [1024, 0, 0]], np.int16), IDENT_T),
           ("random", rng.integers(-32768, 32768, (3, 3)).astype(np.int16), rng.integers(0, 256, 256, dtype=np.uint8)),
           ("camera", utils.raw_ccm(CAMERA), utils.raw_curve("srgb"))]
    for _, m, t in out:
        m.setflags(write=False), t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def table8():
    t = np.random.default_rng(8).integers(0, 256, (4, 256), dtype=np.uint8)
    t.setflags(write=False)
    return t


def _kind(pattern, kind, size):
    """-> (pixel format, raw table or None, the frame pool)."""
    if kind in ("8", "8lut"):
        return pattern, (table8() if kind == "8lut" else None), FM.frame_pool(pattern, size)[:BW.POOL]
    bits = int(kind)
    return BW.wide_name(pattern, bits), BW.tables(bits)[0][1], BW.wide_pool(pattern, bits, size)


def host_rgb(frames, fmt, lut, m=None, t=None, stage=True):
    """The frames as the RGB path is fed them: conditioned, demosaiced and taken through the stage, all in NumPy."""
    pattern = fmt if fmt in RB.PATTERNS else "bayer_" + fmt[8:]
    cond = frames if lut is None else utils.apply_raw_lut(frames, fmt, lut)
    rgb = RB.bayer_to_rgb(cond, pattern)
    return utils.apply_raw_color(rgb, m, t) if stage else rgb


def _front(ctx, fmt, size, frames, ids, first, source):
    ctx.set_slot_calibrations(ids, first=first)
    dev = None
    if source == "upload":
        ctx.upload_frames(frames, first=first)
    elif source == "rows":
        ctx.upload_frames(~frames, first=first)              # what a slot held before is not what is read
        ctx.upload_frame_rows(frames, first=first)
    else:
        ctx.upload_frames(~frames, first=first)              # the slot's own frame is not the one to read
        dev = FM.device_surfaces(frames, "rgb", size, 3) if fmt == "rgb" else BW._surfaces_of(frames, fmt)
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


# ---- 1. the front end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["A", "B"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_front_end_with_a_stage_is_the_rgb_one_on_the_converted_frames(pattern, kind, size):
    """Per source and table form (one table: every slot of the run in the same set, each of the four sets in turn; table per slot: the
    mixed id pattern at odd and even first slots), every form with each of the four stages: undistorted rows, R plane and Lab-b plane
    of a raw context with the stage against an RGB context fed the host-converted frames."""
    fmt, lut, pool = _kind(pattern, kind, size)
    raw, rgb = BW._context(fmt, size, lut), BW._context("rgb", size)
    try:
        assert raw.get_raw_color() is None
        case = 0
        for source in SOURCES:
            forms = [("one table, set %d" % s, [s] * N, None, s) for s in range(FM.N_SETS)] + \
                    [("table per slot", FM.ids_pattern(N), 1 + k % 2, k) for k in range(4)]
            for form, ids, at, k in forms:
                name, m, t = stages()[k]                                                   # every stage meets every form of every source
                first = at if at is not None else 1 + case % 3
                frames = pool[[(7 * case + i) % BW.POOL for i in range(N)]]
                case += 1
                raw.set_raw_color(m, t)
                back = raw.get_raw_color()
                assert np.array_equal(back[0], m) and np.array_equal(back[1], t)
                where = "%s %s, stage %s, source %s, %s, slots [%d, %d)" % (fmt, size, name, source, form, first, first + N)
                got = _front(raw, fmt, size, frames, ids, first, source)
                want = _front(rgb, "rgb", size, host_rgb(frames, fmt, lut, m, t), ids, first, source)
                for what, g, p in zip(("undistorted rows", "R plane", "Lab-b plane"), got, want):
                    assert g.shape == p.shape and np.array_equal(g, p), "%s: %d bytes of the %s differ from the RGB context's" % (
                        where, int((g != p).sum()), what)
        # off again: the plain raw kernels, and what they always gave
        raw.set_raw_color(enable=False)
        assert raw.get_raw_color() is None
        assert (raw.raw_lut() is None) == (kind == "8")                                    # the identity table of the stage was never the context's
        frames = pool[3:3 + N]
        got = _front(raw, fmt, size, frames, [1] * N, 1, "upload")
        want = _front(rgb, "rgb", size, host_rgb(frames, fmt, lut, stage=False), [1] * N, 1, "upload")
        assert all(np.array_equal(g, p) for g, p in zip(got, want)), "%s %s: with the stage removed" % (fmt, size)
    finally:
        raw.close()
        rgb.close()


def test_a_table_set_after_the_stage_is_the_one_the_stage_runs_behind():
    """lt_set_raw_lut / lt_set_raw_lut_wide while a stage is set: the walk with the stage reads the new table."""
    for fmt, one, two in (("bayer_grbg", table8(), utils.raw_lut(8, 250, (1.4, 1, 1.2))), ("bayer12_grbg", BW.tables(12)[0][1], BW.tables(12)[2][1])):
        _, m, t = stages()[3]
        pool = FM.frame_pool(fmt, "A")[:N] if fmt == "bayer_grbg" else BW.wide_pool("bayer_grbg", 12, "A")[3:3 + N]
        raw, rgb = BW._context(fmt, "A", one), BW._context("rgb", "A")
        try:
            raw.set_raw_color(m, t)
            for lut in (two, one) + ((None,) if fmt == "bayer_grbg" else ()):
                raw.set_raw_lut(lut)
                got = _front(raw, fmt, "A", pool, FM.ids_pattern(N), 1, "upload")
                want = _front(rgb, "rgb", "A", host_rgb(pool, fmt, lut, m, t), FM.ids_pattern(N), 1, "upload")
                assert all(np.array_equal(g, p) for g, p in zip(got, want)), fmt
        finally:
            raw.close()
            rgb.close()


# ---- 2. the row conversion ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_bayer_to_rgb_color_is_the_numpy_definition(kind):
    """lt_raw_to_rgb_color, dense: the 16-column body (W = 64) and the any-width one (W = 66), every pattern, the stages in turn."""
    for p, pattern in enumerate(PATTERNS):
        for size in ("A", "B"):
            fmt, lut, pool = _kind(pattern, kind, size)
            frames = pool[:4]
            name, m, t = stages()[(p + "AB".index(size) + KINDS.index(kind)) % 4]
            got = utils.bayer_to_rgb_color(frames, fmt, lut, m, t)
            assert got.shape == frames.shape + (3,) and np.array_equal(got, host_rgb(frames, fmt, lut, m, t)), (fmt, size, name)
            one = utils.bayer_to_rgb_color(frames[3], fmt)                                  # nothing given: the plain conversion
            plain_lut = None if kind in ("8", "8lut") else utils.raw_lut(bits=int(kind))
            assert np.array_equal(one, host_rgb(frames[3], fmt, plain_lut, stage=False)), (fmt, size)
            half = utils.bayer_to_rgb_color(frames[2], fmt, lut, curve=t)                   # one of the two: the other is the identity
            assert np.array_equal(half, host_rgb(frames[2], fmt, lut, None, t)), (fmt, size)


@pytest.mark.parametrize("size", ["A", "B"])
@pytest.mark.parametrize("kind", KINDS)
def test_shown_camera_frame_is_the_converted_frame(kind, size):
    """The slot's RGB camera frame of a raw context with a stage against NumPy: whole uploads (dense: the 16-column body at W = 64) and
    attached surfaces (pitch W + 5 / 2 W + 6 at size B: the any-width body), every pattern, the stages in turn."""
    w, h = FM.SIZES[size]
    n, first = 3, 1
    q = FM.calibration_sets(size)[0]                         # the identity: every row is read
    for p, pattern in enumerate(PATTERNS):
        fmt, lut, pool = _kind(pattern, kind, size)
        name, m, t = stages()[(p + 1 + "AB".index(size)) % 4]
        c = _native.Context((w, h), (w, h), q["cam_matrix"], q["dist_coeffs"], q["M"], capacity=n + 1)
        try:
            c.set_input_format(fmt)
            if lut is not None:
                c.set_raw_lut(lut)
            c.set_raw_color(m, t)
            c.overlay_configure(np.linalg.inv(q["M"]))
            frames = pool[:n]
            c.upload_frames(frames, first=first)
            got = BW._read_back(c, n, h, w, first)
            assert np.array_equal(got, host_rgb(frames, fmt, lut, m, t)), ("lt_upload_frames", fmt, size, name)
            other = pool[10:10 + n]
            dev = BW._wide_surfaces(other, fmt, padded=size == "B") if fmt in _native.BAYER_WIDE_FORMATS else BW._narrow_surfaces(other, fmt, padded=size == "B")
            try:
                keep = c.attach_device_frames(dev, first=first)
                c.mask_run(n, first=first)
                c.device_frames_rest(n, first=first)
                got = BW._read_back(c, n, h, w, first)
                del keep
                assert np.array_equal(got, host_rgb(other, fmt, lut, m, t)), ("device_frames_rest", fmt, size, name)
            finally:
                dev.owner.close()
        finally:
            c.close()


# ---- 3. trackers and groups at the reference calibration ----------------------------------------------------------------------------------
def _get_state(t):
    s = t.get_state()
    s.pop("pixel_format", None), s.pop("yuv_matrix", None)
    assert "raw_ccm" not in s and "raw_curve" not in s and "raw_lut" not in s
    return s


def _same(a, b):
    assert _get_state(a) == _get_state(b) and BW._state(a) == BW._state(b)


@functools.lru_cache(maxsize=None)
def _scenes(pattern):
    """Six rendered scenes, mosaicked on the host, and two stages mild enough that the lane is still found: a camera-like matrix with
    a gentle curve, and a second one."""
    r = synth.SceneRenderer()
    mos = RB.rgb_to_bayer(np.stack([r.render(s)[0] for s in range(6)]), pattern)
    mos.setflags(write=False)
    one = (utils.raw_ccm([[1.3, -0.2, -0.1], [-0.1, 1.2, -0.1], [0.0, -0.2, 1.2]]), utils.raw_curve(1.1))
    two = (utils.raw_ccm([[1.1, -0.1, 0.0], [0.0, 1.0, 0.0], [0.0, -0.1, 1.1]]), utils.raw_curve(1.0))
    return mos, one, two


@pytest.mark.parametrize("pattern,bits", [("bayer_gbrg", 8), ("bayer_grbg", 12)])
def test_process_and_process_batch_equal_the_rgb_trackers(pattern, bits):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    mos, (m, t), _ = _scenes(pattern)
    if bits == 8:
        fmt, raw, lut = pattern, mos, utils.raw_lut(0, 250, (1.02, 1, 0.98))
    else:
        fmt, raw, lut = BW.wide_name(pattern, bits), mos.astype(np.uint16) << (bits - 8), None
    conv = host_rgb(raw, fmt, lut if lut is not None else utils.raw_lut(bits=bits), m, t)
    pair = lambda: (LaneTracker(**cal, pixel_format=fmt, raw_lut=lut, raw_ccm=m, raw_curve=t), LaneTracker(**cal))
    a, b = pair()
    try:                                                     # process()
        assert np.array_equal(a.raw_ccm, m) and np.array_equal(a.raw_curve, t) and np.array_equal(a._ctx.get_raw_color()[0], m)
        for k in range(3):
            oa, ob = a.process(raw[k]), b.process(conv[k])
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
        oa, ob = a.process_batch(raw), b.process_batch(conv)
        assert len(oa) == 6 and all(np.array_equal(x, y) for x, y in zip(oa, ob))
        _same(a, b)
        assert b.get_success_ratio() == (1.0, 6, 6)
    finally:
        a.close()
        b.close()


def test_process_stream_with_a_stage_change_between_windows_and_the_stage_off():
    cal = calib.reference_calibration()
    pattern = "bayer_rggb"
    mos, one, two = _scenes(pattern)
    conv = np.concatenate([host_rgb(mos[:3], pattern, None, *one), host_rgb(mos[3:5], pattern, None, *two), host_rgb(mos[5:], pattern, None, stage=False)])
    dev = BW._narrow_surfaces(mos, pattern)
    a, b, plain = LaneTracker(**cal, pixel_format=pattern, raw_ccm=one[0], raw_curve=one[1]), LaneTracker(**cal), LaneTracker(**cal, pixel_format=pattern)
    try:
        for w_, (oa, ob) in enumerate(zip(a.process_stream([dev[:2], dev[2:3]]), b.process_stream([conv[:2], conv[2:3]]))):       # device frames
            assert len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w_
        _same(a, b)
        a.set_raw_color(*two)                                # between windows: the results switch at the window's edge
        assert np.array_equal(a.raw_ccm, two[0]) and np.array_equal(a._ctx.get_raw_color()[1], two[1])
        for w_, (oa, ob) in enumerate(zip(a.process_stream([mos[3:5]]), b.process_stream([conv[3:5]]))):                           # host frames
            assert len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w_
        _same(a, b)
        a.set_raw_color()                                    # off: the plain raw tracker's output again
        assert a.raw_ccm is None and a._ctx.get_raw_color() is None
        plain.set_state(a.get_state())
        oa, ob, op = a.process(mos[5]), b.process(conv[5]), plain.process(mos[5])
        assert np.array_equal(oa, ob) and np.array_equal(oa, op)
        _same(a, b)
        assert a.counter == 6 and b.success >= 5
    finally:
        a.close()
        b.close()
        plain.close()
        dev.owner.close()


@pytest.mark.parametrize("pattern,bits", [("bayer_bggr", 8), ("bayer_gbrg", 10)])
def test_a_group_equals_the_rgb_trackers(pattern, bits):
    cal = calib.reference_calibration()
    mos, (m, t), two = _scenes(pattern)
    if bits == 8:
        fmt, raw = pattern, mos
    else:
        fmt, raw = BW.wide_name(pattern, bits), mos.astype(np.uint16) << (bits - 8)
    lut = None if bits == 8 else utils.raw_lut(bits=bits)
    conv = host_rgb(raw, fmt, lut, m, t)
    g, solos = LaneTrackerGroup(2, **cal, pixel_format=fmt, raw_ccm=m, raw_curve=t), [LaneTracker(**cal) for _ in range(2)]
    try:                                                     # a group of two: stream 1 runs two frames ahead
        assert np.array_equal(g.raw_ccm, m) and np.array_equal(g._ctx.get_raw_color()[1], t)
        for k in range(3):
            outs = g.process([raw[k], raw[k + 2]])
            for i, f in enumerate((k, k + 2)):
                assert np.array_equal(outs[i], solos[i].process(conv[f])), (k, i)
                assert _get_state(g.trackers[i]) == _get_state(solos[i]), (k, i)
        with pytest.raises(RuntimeError):
            g.trackers[0].set_raw_color(*two)
        g.set_raw_color(*two)                                # one stage for all the streams, changed between calls
        conv2 = host_rgb(raw, fmt, lut, *two)
        outs = g.process([raw[3], raw[5]])
        for i, f in enumerate((3, 5)):
            assert np.array_equal(outs[i], solos[i].process(conv2[f])), i
            assert _get_state(g.trackers[i]) == _get_state(solos[i]), i
        assert solos[0].success == 4
    finally:
        g.close()
        for s in solos:
            s.close()


# ---- 4. refusals from the library itself, and memory ----------------------------------------------------------------------------------------
def test_the_library_refuses_a_stage_on_input_that_is_not_raw_bayer():
    w, h = 64, 48
    m, t = stages()[2][1:]
    for fmt in ("rgb", "nv12"):
        c = _native.Context((w, h), (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=2)
        try:
            c.set_input_format(fmt)
            frames = FM.frame_pool(fmt, "A")[:2]
            c.upload_frames(frames)
            c.mask_run(2)
            before = c.download_undistorted(2)
            for enable in (1, 0):
                assert c.lib.lt_set_raw_color(c._h, m.ctypes.data, t.ctypes.data, enable) == -5 and b"raw Bayer" in c.lib.lt_last_error()
            assert c.lib.lt_set_raw_color(c._h, None, None, 1) == -5
            assert c.get_raw_color() is None
            c.mask_run(2)
            assert np.array_equal(c.download_undistorted(2), before)          # nothing changed, nothing was launched in its name
        finally:
            c.close()
    c = _native.Context((w, h), (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=2)
    try:
        out, frame = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8)
        call = lambda layout, hh, lut, entries: c.lib.lt_raw_to_rgb_color(c._h, frame.ctypes.data, hh, w, layout, lut, entries, None, None, out.ctypes.data)
        assert call(0, h, None, 0) == -1 and call(1, h, None, 0) == -1 and call(20, h, None, 0) == -1      # not a raw layout
        assert call(16, h + 1, None, 0) == -1                                                            # an odd height
        assert call(16, h, table8().ctypes.data, 1024) == -1 and b"entries" in c.lib.lt_last_error()
        assert call(32, h, table8().ctypes.data, 256) == -1
        assert not out.any()
        c.set_input_format("bayer_rggb")
        c.set_raw_color(m, t)
        c.set_input_format("rgb")                             # another layout removes the stage
        assert c.get_raw_color() is None
    finally:
        c.close()


def test_contexts_with_a_stage_give_their_memory_back():
    live = lambda: _native.device_cache_stats()["live_bytes"]
    base = live()
    for fmt, lut in (("bayer_bggr", None), ("bayer12_bggr", BW.tables(12)[0][1])):
        c = BW._context(fmt, "A", lut)
        try:
            c.set_raw_color(*stages()[3][1:])
            pool = FM.frame_pool(fmt, "A")[:N] if lut is None else BW.wide_pool("bayer_bggr", 12, "A")[:N]
            _front(c, fmt, "A", pool, [0] * N, 1, "surfaces")
            c.set_raw_color(enable=False)
        finally:
            c.close()
        assert live() == base, fmt
