"""Lens-shading correction of raw Bayer input on the device: the invariant, bit for bit -- whatever a raw Bayer context, tracker or group
with shading map S (and any raw table or colour stage) computes from frames F is what the same object without a map computes from
`utils.apply_raw_shading(F, pattern, S)`, the frames shaded on the host -- for the expansion of the mesh (k_shade_expand), the walks
(k_raw_walk_rows with STAGES 4 .. 7), the row conversions (k_raw_rows_rgb, the same) and everything behind them.

Sizes A (64 x 48) and B (66 x 50) of front_matrix.py: the smallest that hit both the dword-multiple and the odd row bytes, the 16-column
and the any-width body of the row conversion.  Frames: the pools of test_gpu_bayer.py (front_matrix.frame_pool) and of
test_gpu_bayer_wide.py (wide_pool).  Maps: the identity; a 2 x 2 mesh with four unlike corners per colour and unlike pedestals per phase; a
random full-range 5 x 4 mesh; a camera-like 17 x 13 vignette, 1 + 1.5 r^2 times 1 / 1.05 / 1.05 / 1.1 per colour over a pedestal of a
sixteenth of full scale (16 at 8 bits, 256 at 12); tests/test_raw_shading_cpu.py checks, in NumPy alone, that on these frames it changes most
samples and saturates few."""
import functools

import numpy as np
import pytest

import bayer_reference as RB
import front_matrix as FM
import test_gpu_bayer_wide as BW
import test_gpu_raw_color as GC
from lane_tracker_amd import _native, calib, synth, utils
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

PATTERNS = list(RB.PATTERNS)
N = BW.N                                 # slots of a run: ids_pattern(5) = sets 0, 1, 2, 3, 0
SOURCES = GC.SOURCES
KINDS = GC.KINDS                         # 8-bit without a table, 8-bit behind a random table, 10 bits, 12 bits
LONG = 25                                # slots of the long run: 3 frames per walk, the last walk with one


def bits_of(kind):
    return 8 if kind in ("8", "8lut") else int(kind)


def vignette(bits, strength=1.5):
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    g = 1 + strength * (x * x + y * y) / 2                   # r = 1 in the corners
    return utils.raw_shading(np.stack([g, 1.05 * g, 1.05 * g, 1.1 * g]), black_level=16 << (bits - 8), bits=bits)


@functools.lru_cache(maxsize=None)
def maps(bits):
    rng = np.random.default_rng(300 + bits)
    smax = (1 << bits) - 1
    corners = np.array([[[4096, 9000], [2000, 16000]], [[5000, 3000], [12000, 4500]], [[7000, 7500], [3500, 20000]], [[2500, 11000], [6000, 4096]]], np.uint16)
    out = [("identity", utils.RawShading(np.full((4, 2, 2), 4096, np.uint16), np.zeros(4, np.int32))),
           ("corners", utils.RawShading(corners, np.array([0, smax >> 4, smax >> 3, smax >> 5], np.int32))),
           ("random", utils.RawShading(rng.integers(0, 65536, (4, 4, 5)).astype(np.uint16), rng.integers(0, smax + 1, 4).astype(np.int32))),
           ("vignette", vignette(bits))]
    for _, s in out:
        s.mesh.setflags(write=False), s.black.setflags(write=False)
    return out


def _kind(pattern, kind, size):
    """-> (pixel format, raw table or None, the frame pool): test_gpu_raw_color's, the wide pool without its three special frames."""
    fmt, lut, pool = GC._kind(pattern, kind, size)
    return fmt, lut, (pool if bits_of(kind) == 8 else pool[3:])


# ---- 1. the expansion ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["A", "B"])
def test_the_device_expands_the_mesh_into_the_numpy_plane(size):
    """k_shade_expand alone, through lt_get_raw_shading_plane: every pattern, every map, and the largest and a lopsided mesh."""
    rng = np.random.default_rng(5)
    extra = [("64 x 64", utils.RawShading(rng.integers(0, 65536, (4, 64, 64)).astype(np.uint16), np.zeros(4, np.int32))),
             ("2 x 64", utils.RawShading(rng.integers(0, 65536, (4, 64, 2)).astype(np.uint16), np.zeros(4, np.int32))),
             ("all 65535", utils.RawShading(np.full((4, 3, 7), 65535, np.uint16), np.zeros(4, np.int32)))]
    for pattern in PATTERNS:
        for fmt, bits in ((pattern, 8), (BW.wide_name(pattern, 12), 12)):
            c = BW._context(fmt, size)
            try:
                assert c.get_raw_shading() is None
                with pytest.raises(RuntimeError):
                    c.raw_shading_plane()
                for name, s in maps(bits) + extra:
                    c.set_raw_shading(s)
                    back = c.get_raw_shading()
                    assert np.array_equal(back.mesh, s.mesh) and np.array_equal(back.black, s.black), (fmt, name)
                    got = c.raw_shading_plane()
                    assert np.array_equal(got, utils.raw_shading_plane(s, fmt, FM.SIZES[size])), (fmt, size, name)
                c.set_raw_shading(None)
                assert c.get_raw_shading() is None
            finally:
                c.close()


# ---- 2. the front end -------------------------------------------------------------------------------------------------------------------
def _stage(raw, ref, cc):
    m, t = GC.stages()[3][1:] if cc else (None, None)
    for c in (raw, ref):
        c.set_raw_color(m, t, enable=cc)


@pytest.mark.parametrize("size", ["A", "B"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_front_end_with_a_map_is_the_plain_one_on_the_shaded_frames(pattern, kind, size):
    """Per source and table form (one table: every slot of the run in the same set, each of the four sets in turn; table per slot: the
    mixed id pattern at odd and even first slots), every form with each of the four maps, with and without a colour stage: undistorted
    rows, R plane and Lab-b plane of a raw context with the map against the same context without one fed the host-shaded frames."""
    fmt, lut, pool = _kind(pattern, kind, size)
    raw, ref = BW._context(fmt, size, lut), BW._context(fmt, size, lut)
    try:
        case = 0
        for si, source in enumerate(SOURCES):
            forms = [("one table, set %d" % s, [s] * N, None) for s in range(FM.N_SETS)] + \
                    [("table per slot", FM.ids_pattern(N), 1 + k % 2) for k in range(4)]
            for j, (form, ids, at) in enumerate(forms):
                name, s = maps(bits_of(kind))[j % 4]                                       # every map meets every form of every source ...
                cc = (j // 4 + si + PATTERNS.index(pattern)) % 2 == 1                      # ... and a colour stage or none
                first = at if at is not None else 1 + case % 3
                frames = pool[[(7 * case + i) % len(pool) for i in range(N)]]
                case += 1
                _stage(raw, ref, cc)
                raw.set_raw_shading(s)
                where = "%s %s, map %s, colour stage %s, source %s, %s, slots [%d, %d)" % (fmt, size, name, cc, source, form, first, first + N)
                got = BW._front(raw, fmt, frames, ids, first, source)
                want = BW._front(ref, fmt, utils.apply_raw_shading(frames, fmt, s), ids, first, source)
                for what, g, p in zip(("undistorted rows", "R plane", "Lab-b plane"), got, want):
                    assert g.shape == p.shape and np.array_equal(g, p), "%s: %d bytes of the %s differ from the plain context's" % (
                        where, int((g != p).sum()), what)
        # off again: the kernels that ran before, and what they always gave
        raw.set_raw_shading(None)
        assert raw.get_raw_shading() is None
        assert (raw.raw_lut() is None) == (kind == "8")                                    # the identity table of the map was never the context's
        frames = pool[3:3 + N]
        for cc in (True, False):
            _stage(raw, ref, cc)
            got = BW._front(raw, fmt, frames, [1] * N, 1, "upload")
            want = BW._front(ref, fmt, frames, [1] * N, 1, "upload")
            assert all(np.array_equal(g, p) for g, p in zip(got, want)), "%s %s: with the map removed" % (fmt, size)
    finally:
        raw.close()
        ref.close()


# ---- 3. the gains held across the per-frame loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["8lut", "12"])
def test_a_long_run_walks_three_frames_per_thread_with_the_same_gains(kind):
    """25 slots of one set in one launch: 3 frames per walk, the last walk with a single one -- every other run of this file has one."""
    pattern, size = "bayer_gbrg", "B"
    fmt, lut, pool = _kind(pattern, kind, size)
    raw, ref = BW._context(fmt, size, lut, capacity=LONG + 3), BW._context(fmt, size, lut, capacity=LONG + 3)
    try:
        for k, (source, cc, (name, s)) in enumerate((("upload", False, maps(bits_of(kind))[3]), ("surfaces", True, maps(bits_of(kind))[2]))):
            frames = pool[[(5 * k + i) % len(pool) for i in range(LONG)]]
            _stage(raw, ref, cc)
            raw.set_raw_shading(s)
            got = BW._front(raw, fmt, frames, [2] * LONG, 1 + k, source)
            want = BW._front(ref, fmt, utils.apply_raw_shading(frames, fmt, s), [2] * LONG, 1 + k, source)
            for what, g, p in zip(("undistorted rows", "R plane", "Lab-b plane"), got, want):
                bad = sorted(set(np.nonzero((g != p).reshape(LONG, -1).any(axis=1))[0].tolist()))
                assert not bad, "%s, map %s, source %s: the %s of frames %s differ" % (fmt, name, source, what, bad)
    finally:
        raw.close()
        ref.close()


# ---- 4. the order of the settings ---------------------------------------------------------------------------------------------------------
def test_table_stage_and_map_may_be_set_in_any_order():
    """lt_set_raw_lut / lt_set_raw_lut_wide / lt_set_raw_color before or after lt_set_raw_shading: the same result; an 8-bit table taken
    away under a map leaves the identity table behind it."""
    m, t = GC.stages()[3][1:]
    for fmt, one, two in (("bayer_grbg", GC.table8(), utils.raw_lut(8, 250, (1.4, 1, 1.2))), ("bayer12_grbg", BW.tables(12)[0][1], BW.tables(12)[2][1])):
        bits = 8 if fmt == "bayer_grbg" else 12
        s = maps(bits)[3][1]
        pool = FM.frame_pool(fmt, "A")[:N] if bits == 8 else BW.wide_pool("bayer_grbg", 12, "A")[3:3 + N]
        shaded = utils.apply_raw_shading(pool, fmt, s)
        after, before, ref = BW._context(fmt, "A", one), BW._context(fmt, "A"), BW._context(fmt, "A")
        try:
            after.set_raw_shading(s)                             # the map, then stage and table
            for lut in (two, one) + ((None,) if bits == 8 else ()):
                for cc in (True, False):
                    after.set_raw_color(m, t, enable=cc)
                    after.set_raw_lut(lut)
                    before.set_raw_shading(None)                 # table and stage, then the map
                    before.set_raw_lut(lut)
                    before.set_raw_color(m, t, enable=cc)
                    before.set_raw_shading(s)
                    ref.set_raw_lut(lut)
                    ref.set_raw_color(m, t, enable=cc)
                    want = BW._front(ref, fmt, shaded, FM.ids_pattern(N), 1, "upload")
                    for c in (after, before):
                        got = BW._front(c, fmt, pool, FM.ids_pattern(N), 1, "upload")
                        assert all(np.array_equal(g, p) for g, p in zip(got, want)), (fmt, lut is None, cc, c is after)
        finally:
            after.close(), before.close(), ref.close()


# ---- 5. the row conversion ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_bayer_to_rgb_color_with_a_map_is_the_numpy_definition(kind):
    """lt_raw_to_rgb_shaded, dense: the 16-column body (W = 64) and the any-width one (W = 66), every pattern, the maps in turn, with and
    without a colour stage."""
    bits = bits_of(kind)
    for p, pattern in enumerate(PATTERNS):
        for size in ("A", "B"):
            fmt, lut, pool = _kind(pattern, kind, size)
            frames = pool[:3]
            plain_lut = lut if (lut is not None or bits == 8) else utils.raw_lut(bits=bits)
            for k in range(4):
                name, s = maps(bits)[(p + k) % 4]
                cc = (k + "AB".index(size)) % 2 == 1
                m, t = GC.stages()[2 + k % 2][1:] if cc else (None, None)
                got = utils.bayer_to_rgb_color(frames[k % 3], fmt, lut, m, t, shading=s)
                want = GC.host_rgb(utils.apply_raw_shading(frames[k % 3], fmt, s), fmt, plain_lut, m, t, stage=cc)
                assert got.shape == want.shape and np.array_equal(got, want), (fmt, size, name, cc)
            got = utils.bayer_to_rgb_color(frames, fmt, lut, shading=maps(bits)[3][1])    # a stack
            assert np.array_equal(got, GC.host_rgb(utils.apply_raw_shading(frames, fmt, maps(bits)[3][1]), fmt, plain_lut, stage=False)), (fmt, size)


@pytest.mark.parametrize("size", ["A", "B"])
@pytest.mark.parametrize("kind", KINDS)
def test_shown_camera_frame_is_the_shaded_frame_converted(kind, size):
    """The slot's RGB camera frame of a raw context with a map against NumPy: whole uploads (dense: the 16-column body at W = 64) and
    attached surfaces (pitch W + 5 / 2 W + 6 at size B: the any-width body), every pattern, the maps in turn, with and without a stage."""
    w, h = FM.SIZES[size]
    n, first = 3, 1
    bits = bits_of(kind)
    q = FM.calibration_sets(size)[0]                         # the identity: every row is read
    for p, pattern in enumerate(PATTERNS):
        fmt, lut, pool = _kind(pattern, kind, size)
        c = _native.Context((w, h), (w, h), q["cam_matrix"], q["dist_coeffs"], q["M"], capacity=n + 1)
        try:
            c.set_input_format(fmt)
            if lut is not None:
                c.set_raw_lut(lut)
            c.overlay_configure(np.linalg.inv(q["M"]))
            for k, cc in enumerate((False, True)):
                name, s = maps(bits)[(p + 2 * k + 1 + "AB".index(size)) % 4]
                m, t = GC.stages()[3][1:] if cc else (None, None)
                c.set_raw_color(m, t, enable=cc)
                c.set_raw_shading(s)
                frames = pool[6 * k:6 * k + n]
                c.upload_frames(frames, first=first)
                got = BW._read_back(c, n, h, w, first)
                want = GC.host_rgb(utils.apply_raw_shading(frames, fmt, s), fmt, lut, m, t, stage=cc)
                assert np.array_equal(got, want), ("lt_upload_frames", fmt, size, name, cc)
                other = pool[10 + k:10 + k + n]
                dev = BW._wide_surfaces(other, fmt, padded=size == "B") if fmt in _native.BAYER_WIDE_FORMATS else BW._narrow_surfaces(other, fmt, padded=size == "B")
                try:
                    keep = c.attach_device_frames(dev, first=first)
                    c.mask_run(n, first=first)
                    c.device_frames_rest(n, first=first)
                    got = BW._read_back(c, n, h, w, first)
                    del keep
                    want = GC.host_rgb(utils.apply_raw_shading(other, fmt, s), fmt, lut, m, t, stage=cc)
                    assert np.array_equal(got, want), ("device_frames_rest", fmt, size, name, cc)
                finally:
                    dev.owner.close()
        finally:
            c.close()


# ---- 6. trackers and groups at the reference calibration ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scenes(pattern):
    """Six rendered scenes as a lens with one stop of vignetting would leave them on the sensor -- mosaicked on the host, divided by the
    gain -- and the maps that undo it: the right one, and a second, weaker one."""
    r = synth.SceneRenderer()
    mos = RB.rgb_to_bayer(np.stack([r.render(s)[0] for s in range(6)]), pattern)
    one, two = vignette(8, 1.0), vignette(8, 0.5)
    one = utils.RawShading(one.mesh, np.zeros(4, np.int32))
    gain = utils.raw_shading_plane(one, pattern, mos.shape[:0:-1]).astype(np.float64) / 4096
    dark = np.clip(np.rint(mos / gain), 0, 255).astype(np.uint8)
    dark.setflags(write=False)
    return dark, one, two


@pytest.mark.parametrize("pattern,bits", [("bayer_gbrg", 8), ("bayer_grbg", 12)])
def test_process_batch_and_process_stream_equal_the_plain_trackers(pattern, bits):
    cal = calib.reference_calibration()
    dark, one, two = _scenes(pattern)
    if bits == 8:
        fmt, raw, s1, s2 = pattern, dark, one, two
    else:
        fmt, raw = BW.wide_name(pattern, bits), dark.astype(np.uint16) << (bits - 8)
        s1, s2 = one, utils.RawShading(two.mesh, two.black << (bits - 8))
    m, t = utils.raw_ccm([[1.1, -0.1, 0.0], [0.0, 1.0, 0.0], [0.0, -0.1, 1.1]]), utils.raw_curve(1.0)
    a, b = LaneTracker(**cal, pixel_format=fmt, raw_ccm=m, raw_curve=t, raw_shading=s1), LaneTracker(**cal, pixel_format=fmt, raw_ccm=m, raw_curve=t)
    try:
        back = a._ctx.get_raw_shading()
        assert np.array_equal(a.raw_shading.mesh, s1.mesh) and np.array_equal(back.mesh, s1.mesh) and np.array_equal(back.black, s1.black)
        oa, ob = a.process_batch(raw[:3]), b.process_batch(utils.apply_raw_shading(raw[:3], fmt, s1))
        assert len(oa) == 3 and repr(oa) == repr(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob))
        BW._same(a, b)
        assert b.success == 3                                # the comparison is not between two failures
        a.set_raw_shading(s2)                                # between windows: the results switch at the window's edge
        assert np.array_equal(a._ctx.get_raw_shading().black, s2.black)
        shaded = utils.apply_raw_shading(raw[3:], fmt, s2)
        for w_, (oa, ob) in enumerate(zip(a.process_stream([raw[3:5], raw[5:]]), b.process_stream([shaded[:2], shaded[2:]]))):
            assert len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w_
        BW._same(a, b)
        a.set_raw_shading(None)                              # off: the plain tracker's output again
        assert a.raw_shading is None and a._ctx.get_raw_shading() is None
        assert np.array_equal(a.process(raw[0]), b.process(raw[0]))
        BW._same(a, b)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("pattern,bits", [("bayer_bggr", 8), ("bayer_rggb", 10)])
def test_a_group_tick_equals_the_plain_groups(pattern, bits):
    cal = calib.reference_calibration()
    dark, one, two = _scenes(pattern)
    if bits == 8:
        fmt, raw, s1, s2 = pattern, dark, one, two
    else:
        fmt, raw = BW.wide_name(pattern, bits), dark.astype(np.uint16) << (bits - 8)
        s1, s2 = one, utils.RawShading(two.mesh, two.black << (bits - 8))
    g, ref = LaneTrackerGroup(2, **cal, pixel_format=fmt, raw_shading=s1), LaneTrackerGroup(2, **cal, pixel_format=fmt)
    try:                                                     # groups of two: stream 1 runs two frames ahead
        assert np.array_equal(g.raw_shading.mesh, s1.mesh) and np.array_equal(g._ctx.get_raw_shading().mesh, s1.mesh)
        shaded = utils.apply_raw_shading(raw, fmt, s1)
        for k in range(2):
            oa, ob = g.process([raw[k], raw[k + 2]]), ref.process([shaded[k], shaded[k + 2]])
            assert repr(oa) == repr(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob)), k
            for i in range(2):
                BW._same(g.trackers[i], ref.trackers[i])
        with pytest.raises(RuntimeError):
            g.trackers[0].set_raw_shading(s2)
        g.set_raw_shading(s2)                                # one map for all the streams, changed between calls
        shaded = utils.apply_raw_shading(raw, fmt, s2)
        oa, ob = g.process([raw[2], raw[4]]), ref.process([shaded[2], shaded[4]])
        assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
        for i in range(2):
            BW._same(g.trackers[i], ref.trackers[i])
        assert ref.trackers[0].success == 3
    finally:
        g.close()
        ref.close()


# ---- 7. refusals from the library itself, and memory ----------------------------------------------------------------------------------------
def test_the_library_refuses_a_map_it_cannot_take():
    w, h = 64, 48
    s = maps(8)[3][1]
    mesh, black = np.ascontiguousarray(s.mesh), np.ascontiguousarray(s.black)
    for fmt in ("rgb", "nv12"):
        c = _native.Context((w, h), (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=2)
        try:
            c.set_input_format(fmt)
            for enable in (1, 0):
                assert c.lib.lt_set_raw_shading(c._h, mesh.ctypes.data, 17, 13, black.ctypes.data, enable) == -5 and b"raw Bayer" in c.lib.lt_last_error()
            assert c.get_raw_shading() is None
        finally:
            c.close()
    c = _native.Context((w, h), (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=2)
    try:
        c.set_input_format("bayer_rggb")
        big = np.full((4, 65, 65), 4096, np.uint16)
        call = lambda mw, mh, b: c.lib.lt_set_raw_shading(c._h, big.ctypes.data, mw, mh, None if b is None else np.array(b, np.int32).ctypes.data, 1)
        for mw, mh in ((1, 2), (2, 1), (65, 2), (2, 65), (0, 0), (-3, 4)):
            assert call(mw, mh, None) == -1 and b"nodes" in c.lib.lt_last_error(), (mw, mh)
        assert call(2, 2, [0, 0, 0, 256]) == -1 and b"black" in c.lib.lt_last_error()
        assert call(2, 2, [-1, 0, 0, 0]) == -1
        assert c.lib.lt_set_raw_shading(c._h, None, 2, 2, None, 1) == -1
        assert c.get_raw_shading() is None
        assert call(2, 2, [0, 0, 0, 255]) == 0 and c.get_raw_shading().black.tolist() == [0, 0, 0, 255]      # (black = NULL: zeros)
        assert call(64, 64, None) == 0 and c.get_raw_shading().black.tolist() == [0, 0, 0, 0]
        c.set_input_format("bayer12_rggb")                    # another layout removes the map
        assert c.get_raw_shading() is None
        assert call(2, 2, [0, 0, 0, 4095]) == 0 and call(2, 2, [0, 0, 0, 4096]) == -1
        c.set_input_format("rgb")
        assert c.get_raw_shading() is None
        out, frame = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8)
        conv = lambda layout, hh, mw, b: c.lib.lt_raw_to_rgb_shaded(c._h, frame.ctypes.data, hh, w, layout, None, 0, None, None, big.ctypes.data, mw, 2,
                                                                    None if b is None else np.array(b, np.int32).ctypes.data, out.ctypes.data)
        assert conv(0, h, 2, None) == -1 and conv(20, h, 2, None) == -1                                   # not a raw layout
        assert conv(16, h + 1, 2, None) == -1 and conv(16, h, 1, None) == -1 and conv(16, h, 2, [0, 0, 300, 0]) == -1
        assert not out.any()
    finally:
        c.close()


def test_the_gain_plane_is_allocated_by_the_first_set_and_freed_on_removal():
    live = lambda: _native.device_cache_stats()["live_bytes"]
    base = live()
    for fmt, lut in (("bayer_bggr", None), ("bayer12_bggr", BW.tables(12)[0][1])):
        bits = 8 if lut is None else 12
        c = BW._context(fmt, "A", lut)
        try:
            pool = FM.frame_pool(fmt, "A")[:N] if lut is None else BW.wide_pool("bayer_bggr", 12, "A")[3:3 + N]
            BW._front(c, fmt, pool, [0] * N, 1, "surfaces")
            without = live()                                  # a context that never set a map has allocated nothing for one
            c.set_raw_shading(maps(bits)[3][1])
            with_map = live()
            assert with_map > without
            c.set_raw_shading(maps(bits)[2][1])               # another map: the same plane
            assert live() == with_map
            BW._front(c, fmt, pool, [0] * N, 1, "surfaces")
            c.set_raw_shading(None)
            assert live() == without + (1024 if bits == 8 else 0)          # the plane is gone (8 bits: the identity table's 1 KB block stays the context's)
        finally:
            c.close()
        assert live() == base, fmt
