"""MIPI-packed RAW10 / RAW12 Bayer on the device: the invariant, bit for bit -- whatever a context, tracker or group in 'bayer10p_P' /
'bayer12p_P' with table L (and, optionally, a colour stage and a shading map) computes from packed frames F is what the 'bayer10_P' /
'bayer12_P' object with the same table, stage and map computes from `utils.unpack_raw(F, fmt)` -- for the packed walks (k_mipi_walk_rows),
the packed row conversions (k_mipi_rows_rgb) and everything behind them; and `utils.bayer_to_rgb` on packed frames against the NumPy
demosaic of tests/bayer_reference.py, so that one leg rests on a definition that is not device code.

Sizes: 64 x 48 for both packings (row bytes 80 / 96, dword multiples: the 16-column body of the row conversion), 68 x 50 for RAW10 (85 row
bytes) and 66 x 50 for RAW12 (99): odd row bytes, the site-wise body, every byte alignment of a window row.  front_matrix.py has no
68 x 50, so the four calibration sets of a size are built here the way front_matrix.calibration_sets builds them.  Runs: five slots with
mixed calibration sets, capacity 8; sources upload, rows, surfaces (pitch = row bytes + 3, the plane at byte 1 of its block) and dense
surfaces whose last row ends on the last byte of the block.  Frames: all zero, all maximum, only the low bits set, only the high bytes
set, a frame whose value follows x % 4 and y % 2 (any mix-up of a sample's low bits shows), random samples.  Tables: random with
independently drawn rows, the default, raw_lut(.., 'srgb', bits=NN)."""
import functools

import numpy as np
import pytest

import bayer_reference as RB
import front_matrix as FM
import test_gpu_bayer_wide as BW
import test_gpu_raw_color as GC
import test_gpu_raw_shading as GS
from lane_tracker_amd import _native, calib, utils
from lane_tracker_amd.device import DeviceBuffer, DeviceFrames, pack_host_frames
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

PATTERNS = list(RB.PATTERNS)
N, CAPACITY, POOL = 5, 8, 12
SIZES = {(10, "even"): (64, 48), (10, "odd"): (68, 50), (12, "even"): (64, 48), (12, "odd"): (66, 50)}
SOURCES = ("upload", "rows", "surfaces", "surfaces to the last byte")
COMBOS = ((False, False), (True, False), (False, True), (True, True))        # (colour stage, shading map)


def names(pattern, bits):
    """-> (the packed format, the 16-bit format) of an 8-bit pattern's name."""
    return "bayer%dp_%s" % (bits, pattern[6:]), "bayer%d_%s" % (bits, pattern[6:])


def row_bytes(bits, w):
    return w * 5 // 4 if bits == 10 else w * 3 // 2


def calibration_sets(wh):
    """front_matrix.calibration_sets for any size: the identity, taps outside the image, a narrow run of rows, a general affine view."""
    w, h = wh
    cx, cy = (w - 1) / 2, (h - 1) / 2
    K = lambda fx, fy, x, y: np.array([[fx, 0, x], [0, fy, y], [0, 0, 1.0]])
    M = lambda a, b, tx, c, d, ty: np.array([[a, b, tx], [c, d, ty], [0, 0, 1.0]])
    return [dict(cam_matrix=np.eye(3), dist_coeffs=np.zeros(5), M=np.eye(3)),
            dict(cam_matrix=K(40, 40, cx, cy), dist_coeffs=np.array([0.3, 0, 0.01, 0, 0]), M=M(1, 0, -9.5, 0, 1, 6.25)),
            dict(cam_matrix=K(55, 50, cx + 2, cy - 1), dist_coeffs=np.array([-0.2, 0.05, 0, 0.01, 0]), M=M(1, 0, 0, 0, 2, -30.5)),
            dict(cam_matrix=K(48, 48, cx - 3, cy + 2), dist_coeffs=np.array([0.1, 0, 0, 0, 0]), M=M(1.1, 0.05, -4.25, 0.02, 1.2, -3.5))]


def _context(fmt, wh, lut=None, capacity=CAPACITY):
    sets = calibration_sets(wh)
    c = _native.Context(wh, wh, sets[0]["cam_matrix"], sets[0]["dist_coeffs"], sets[0]["M"], capacity=capacity)
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


@functools.lru_cache(maxsize=None)
def pool(bits, wh):
    """POOL frames of samples, uint16 (POOL, H, W): 0 all zero, 1 all maximum, 2 only low bits, 3 only high bytes, 4 following x % 4 and
    y % 2, the rest random; shared, never changed."""
    w, h = wh
    rng = np.random.default_rng(5000 + 100 * bits + w)
    low = (1 << (bits - 8)) - 1
    out = rng.integers(0, 1 << bits, (POOL, h, w), dtype=np.uint16)
    out[0] = 0
    out[1] = (1 << bits) - 1
    out[2] = rng.integers(0, low + 1, (h, w), dtype=np.uint16)
    out[3] = rng.integers(0, 256, (h, w), dtype=np.uint16) << (bits - 8)
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    out[4] = (((x % 4) * 64 + (y % 2) * 32 + 5) << (bits - 8)) | ((x % 4 + 3 * (y % 2)) & low)
    assert (out >> bits == 0).all() and len({int(v) & low for v in out[4, 0, :4]}) == min(4, low + 1)
    out.setflags(write=False)
    return out


def _packed_surfaces(frames, fmt, padded):
    """Pitch = row bytes + 3 and the plane at byte 1 of its block; or (not padded) dense from the block's first byte: the last row ends on
    the block's last byte."""
    kw = dict(pitch=frames.shape[-1] + 3, offset=1) if padded else {}
    block, surf, size, single = pack_host_frames(frames, fmt, fill=FM.FILL, **kw)
    assert block.nbytes == (1 if padded else 0) + int(surf["pitch"][0]) * (frames.shape[0] * frames.shape[1] - 1) + frames.shape[-1]
    buf = DeviceBuffer(block.nbytes).copy_from_host(block)
    surf["plane"][:, :1] += np.uint64(buf.ptr)
    return DeviceFrames(surf, size, fmt, owner=buf, single=single)


def _surfaces_of(frames, fmt, padded=True):
    return _packed_surfaces(frames, fmt, padded) if fmt in _native.BAYER_PACKED_FORMATS else BW._wide_surfaces(frames, fmt, padded)


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
        dev = _surfaces_of(frames, fmt, padded=source == "surfaces")
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


def _set_stages(ctxs, bits, cc, ls, k):
    m, t = GC.stages()[2 + k % 2][1:] if cc else (None, None)
    s = GS.maps(bits)[1 + k % 3][1] if ls else None
    for c in ctxs:
        c.set_raw_color(m, t, enable=cc)
        c.set_raw_shading(s)
    return m, t, s


# ---- 1. the front end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["even", "odd"])
@pytest.mark.parametrize("bits", (10, 12))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_packed_front_end_is_the_16_bit_one_on_the_unpacked_frames(pattern, bits, size):
    """Per source, table form (one table: every slot of the run in one set; table per slot: the mixed id pattern, at an odd and an even
    first slot in turn) and stage combination (the table alone, with the colour stage, with a shading map, with both), the tables taken in
    turn: undistorted rows, R plane and Lab-b plane of a packed context on F against the 16-bit context on unpack_raw(F)."""
    wh = SIZES[bits, size]
    fmt, wide = names(pattern, bits)
    words = pool(bits, wh)
    packed = utils.pack_raw(words, fmt)
    assert packed.shape == (POOL, wh[1], row_bytes(bits, wh[0])) and np.array_equal(utils.unpack_raw(packed, fmt), words)
    a, b = _context(fmt, wh), _context(wide, wh)
    try:
        assert a.input_format()[0] == fmt and np.array_equal(a.raw_lut(), utils.raw_lut(bits=bits))          # the default, installed with the format
        case = 0
        for source in SOURCES:
            for cc, ls in COMBOS:
                forms = [("one table, set %d" % (case % FM.N_SETS), [case % FM.N_SETS] * N, 1 + case % 3), ("table per slot", FM.ids_pattern(N), 1 + case % 2)]
                for form, ids, first in forms:
                    name, lut = BW.tables(bits)[case % 3]
                    pick = [(5 * case + i) % POOL for i in range(N)]                          # (case 0: the five special frames)
                    case += 1
                    for c in (a, b):
                        c.set_raw_lut(lut)
                    _set_stages((a, b), bits, cc, ls, case)
                    where = "%s %dx%d, table %s, colour stage %s, map %s, source %s, %s, slots [%d, %d)" % (fmt, wh[0], wh[1], name, cc, ls, source, form, first, first + N)
                    got = _front(a, fmt, packed[pick], ids, first, source)
                    want = _front(b, wide, utils.unpack_raw(packed[pick], fmt), ids, first, source)
                    for what, g, p in zip(("undistorted rows", "R plane", "Lab-b plane"), got, want):
                        assert g.shape == p.shape and np.array_equal(g, p), "%s: %d bytes of the %s differ from the 16-bit context's" % (
                            where, int((g != p).sum()), what)
                    assert got[0].any()                                                      # not two empty results
    finally:
        a.close()
        b.close()


# ---- 2. the row conversion ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["even", "odd"])
@pytest.mark.parametrize("bits", (10, 12))
def test_bayer_to_rgb_on_packed_frames_is_the_numpy_demosaic(bits, size):
    """lt_raw_to_rgb_color / _shaded on dense packed rows -- the 16-column body at W = 64, the site-wise one at W = 68 / 66 -- against
    tests/bayer_reference.py on the unpacked, conditioned frames: every pattern, every frame of the pool, the tables in turn; then with a
    colour stage and with a shading map against the NumPy definitions of those."""
    wh = SIZES[bits, size]
    words = pool(bits, wh)
    for p, pattern in enumerate(PATTERNS):
        fmt, wide = names(pattern, bits)
        packed = utils.pack_raw(words, fmt)
        for k, (name, lut) in enumerate(BW.tables(bits)):
            got = utils.bayer_to_rgb(packed, fmt, lut)
            want = RB.bayer_to_rgb(utils.apply_raw_lut(words, wide, lut), pattern)
            assert got.shape == want.shape == (POOL, wh[1], wh[0], 3) and got.dtype == np.uint8
            assert np.array_equal(got, want), "%s %dx%d, table %s: frames %s differ" % (
                fmt, wh[0], wh[1], name, sorted(set(np.nonzero((got != want).reshape(POOL, -1).any(axis=1))[0].tolist())))
        one = utils.bayer_to_rgb(packed[5], fmt)                                             # no table given: the default
        assert np.array_equal(one, RB.bayer_to_rgb(utils.apply_raw_lut(words[5], wide, utils.raw_lut(bits=bits)), pattern))
        lut = BW.tables(bits)[0][1]
        m, t = GC.stages()[2 + p % 2][1:]
        s = GS.maps(bits)[1 + p % 3][1]
        f = packed[4:8]
        assert np.array_equal(utils.bayer_to_rgb_color(f, fmt, lut, m, t), GC.host_rgb(words[4:8], wide, lut, m, t)), (fmt, "colour stage")
        shaded = utils.apply_raw_shading(words[4:8], wide, s)
        assert np.array_equal(utils.bayer_to_rgb_color(f, fmt, lut, shading=s), GC.host_rgb(shaded, wide, lut, stage=False)), (fmt, "map")
        assert np.array_equal(utils.bayer_to_rgb_color(f, fmt, lut, m, t, shading=s), GC.host_rgb(shaded, wide, lut, m, t)), (fmt, "both")


@pytest.mark.parametrize("size", ["even", "odd"])
@pytest.mark.parametrize("bits", (10, 12))
def test_shown_camera_frame_is_the_16_bit_contexts(bits, size):
    """The slot's RGB camera frame of a packed context against the 16-bit context's and against NumPy: whole uploads (dense staging
    frames), row runs that include rows 0 and H - 1 over what a former upload left, and attached surfaces, padded (any byte) and dense --
    every pattern, the stage combinations in turn."""
    w, h = wh = SIZES[bits, size]
    n, first = 3, 1
    q = calibration_sets(wh)[0]                              # the identity: every row is read
    words = pool(bits, wh)
    runs = np.array((0, 3, h - 5, h), np.int32)
    for p, pattern in enumerate(PATTERNS):
        fmt, wide = names(pattern, bits)
        lut = BW.tables(bits)[p % 3][1]
        mk = lambda: _native.Context(wh, wh, q["cam_matrix"], q["dist_coeffs"], q["M"], capacity=n + 1)
        a, b = mk(), mk()
        try:
            for c, f in ((a, fmt), (b, wide)):
                c.set_input_format(f)
                c.set_raw_lut(lut)
                c.overlay_configure(np.linalg.inv(q["M"]))
            for k, (cc, ls) in enumerate(COMBOS):
                m, t, s = _set_stages((a, b), bits, cc, ls, p + k)
                frames, fill = words[[(3 * k + i) % POOL for i in range(n)]], words[[(3 * k + 5 + i) % POOL for i in range(n)]]
                show = lambda f: GC.host_rgb(f if s is None else utils.apply_raw_shading(f, wide, s), wide, lut, m, t, stage=cc)
                where = (fmt, wh, cc, ls)
                a.upload_frames(utils.pack_raw(fill, fmt), first=first)
                b.upload_frames(fill, first=first)
                got, ref = BW._read_back(a, n, h, w, first), BW._read_back(b, n, h, w, first)
                assert np.array_equal(got, ref) and np.array_equal(got, show(fill)), ("lt_upload_frames",) + where
                pf = utils.pack_raw(frames, fmt)
                keep = [a.upload_frame_rows(pf, first=first, enqueue=True), b.upload_frame_rows(frames, first=first, enqueue=True)]
                a.mask_run(n, first=first)
                b.mask_run(n, first=first)
                keep += [a.upload_frame_rest(pf, first=first, rows=runs.ctypes.data), b.upload_frame_rest(frames, first=first, rows=runs.ctypes.data)]
                held = show(fill)
                for lo, hi in ((0, 3), (h - 5, h)):
                    held[:, lo:hi] = show(frames)[:, lo:hi]
                got, ref = BW._read_back(a, n, h, w, first), BW._read_back(b, n, h, w, first)
                del keep
                assert np.array_equal(got, ref) and np.array_equal(got, held), ("rows + rest over two runs",) + where
                for padded in (True, False):
                    da, db = _surfaces_of(utils.pack_raw(frames, fmt), fmt, padded), _surfaces_of(frames, wide, padded)
                    try:
                        for c, d in ((a, da), (b, db)):
                            keep = c.attach_device_frames(d, first=first)
                            c.mask_run(n, first=first)
                            c.device_frames_rest(n, first=first)
                            del keep
                        got, ref = BW._read_back(a, n, h, w, first), BW._read_back(b, n, h, w, first)
                        assert np.array_equal(got, ref) and np.array_equal(got, show(frames)), ("device_frames_rest", padded) + where
                    finally:
                        da.owner.close()
                        db.owner.close()
        finally:
            a.close()
            b.close()


# ---- 3. trackers and groups at the reference calibration ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,bits", [("bayer_gbrg", 10), ("bayer_grbg", 12)])
def test_process_and_process_batch_equal_the_16_bit_trackers(pattern, bits):
    """Annotated frames, records and states of a packed tracker against the 16-bit tracker on the unpacked frames: host frames (the slots'
    staging frames and the 16-column row conversion at W = 1280) and attached surfaces at pitch = row bytes + 3 from byte 1 (the site-wise
    one), the table alone and then with a colour stage and a shading map."""
    cal = calib.reference_calibration()
    fmt, wide = names(pattern, bits)
    raw, one, two = BW._scenes(pattern, bits)[:3]
    packed = utils.pack_raw(raw, fmt)
    a, b = LaneTracker(**cal, pixel_format=fmt, raw_lut=one), LaneTracker(**cal, pixel_format=wide, raw_lut=one)
    try:
        assert a.pixel_format == fmt and np.array_equal(a._ctx.raw_lut(), one)
        oa, ob = a.process(packed[0]), b.process(raw[0])
        assert oa.shape == ob.shape and np.array_equal(oa, ob)
        oa, ob = a.process_batch(packed[1:4]), b.process_batch(raw[1:4])
        assert len(oa) == 3 and all(np.array_equal(x, y) for x, y in zip(oa, ob))
        BW._same(a, b)
        assert b.success == 4                                # the comparison is not between two failures
        m, t = utils.raw_ccm([[1.1, -0.1, 0.0], [0.0, 1.0, 0.0], [0.0, -0.1, 1.1]]), utils.raw_curve(1.0)
        s = utils.RawShading(GS.vignette(bits, 0.2).mesh, np.zeros(4, np.int32))
        for t_ in (a, b):
            t_.set_raw_lut(two)
            t_.set_raw_color(m, t)
            t_.set_raw_shading(s)
        da = DeviceFrames.from_host(packed[4:6], fmt, pitch=packed.shape[-1] + 3, offset=1)
        db = BW._wide_surfaces(raw[4:6], wide)
        try:
            oa, ob = a.process_batch(da), b.process_batch(db)
            assert len(oa) == 2 and all(np.array_equal(x, y) for x, y in zip(oa, ob))
            BW._same(a, b)
        finally:
            da.owner.close()
            db.owner.close()
        for w_, (oa, ob) in enumerate(zip(a.process_stream([packed[:2], packed[2:3]]), b.process_stream([raw[:2], raw[2:3]]))):
            assert len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w_
        BW._same(a, b)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("pattern,bits", [("bayer_bggr", 10), ("bayer_rggb", 12)])
def test_a_group_tick_equals_the_16_bit_groups(pattern, bits):
    cal = calib.reference_calibration()
    fmt, wide = names(pattern, bits)
    raw, one, two = BW._scenes(pattern, bits)[:3]
    packed = utils.pack_raw(raw, fmt)
    m, t = utils.raw_ccm([[1.1, -0.1, 0.0], [0.0, 1.0, 0.0], [0.0, -0.1, 1.1]]), utils.raw_curve(1.0)
    g, ref = LaneTrackerGroup(2, **cal, pixel_format=fmt, raw_lut=one), LaneTrackerGroup(2, **cal, pixel_format=wide, raw_lut=one)
    try:                                                     # groups of two: stream 1 runs two frames ahead
        for k in range(2):
            oa, ob = g.process([packed[k], packed[k + 2]]), ref.process([raw[k], raw[k + 2]])
            assert repr(oa) == repr(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob)), k
            for i in range(2):
                BW._same(g.trackers[i], ref.trackers[i])
        for x in (g, ref):
            x.set_raw_lut(two)
            x.set_raw_color(m, t)
        oa, ob = g.process([packed[2], packed[4]]), ref.process([raw[2], raw[4]])
        assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
        for i in range(2):
            BW._same(g.trackers[i], ref.trackers[i])
        assert ref.trackers[0].success == 3
    finally:
        g.close()
        ref.close()


# ---- 4. refusals from the library itself ------------------------------------------------------------------------------------------------
def test_the_library_refuses_what_the_packed_layouts_cannot_take():
    def ctx(w, h):
        return _native.Context((w, h), (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=2)
    for (w, h), layout, ok in (((66, 50), 36, False), ((66, 50), 52, True), ((68, 50), 36, True), ((67, 50), 52, False), ((68, 49), 36, False)):
        c = ctx(w, h)
        try:
            rc = c.lib.lt_set_input_format(c._h, layout, None)
            assert (rc == 0) == ok, (w, h, layout, rc, c.lib.lt_last_error())
            if not ok:
                assert rc == -1 and c.input_format()[0] == "rgb"
                assert (b"multiple of 4" in c.lib.lt_last_error()) == (layout == 36 and w % 4 == 2 and h % 2 == 0 and h >= 4)
        finally:
            c.close()
    c = ctx(68, 50)
    try:                                                     # a context with an input size: refused, and with the answer these numbers always had there
        c.set_input_size((34, 25))
        for layout in (36, 39, 52, 55):
            assert c.lib.lt_set_input_format(c._h, layout, None) == -1 and b"not resized" in c.lib.lt_last_error(), layout
        assert c.lib.lt_set_input_format(c._h, 32, None) == -5 and c.input_format()[0] == "rgb"
    finally:
        c.close()
    c = ctx(68, 50)
    try:
        c.set_input_format("bayer10p_grbg")
        lut8, lut10, lut12 = np.zeros((4, 256), np.uint8), np.zeros((4, 1024), np.uint8), np.zeros((4, 4096), np.uint8)
        assert c.lib.lt_set_raw_lut(c._h, lut8.ctypes.data) == -5                            # the wide table's call, as for 'bayer10_*'
        assert c.lib.lt_set_raw_lut_wide(c._h, lut12.ctypes.data, 4096) == -1 and c.lib.lt_set_raw_lut_wide(c._h, lut10.ctypes.data, 1024) == 0
        assert c.lib.lt_set_input_size(c._h, 34, 25) == -5                                   # frames of another format are not resized
        blk = np.array([0, 0, 0, 1024], np.int32)
        mesh = np.full((4, 2, 2), 4096, np.uint16)
        assert c.lib.lt_set_raw_shading(c._h, mesh.ctypes.data, 2, 2, blk.ctypes.data, 1) == -1 and b"black" in c.lib.lt_last_error()
        out, words, rows = np.zeros((50, 68, 3), np.uint8), np.zeros((50, 68), np.uint16), np.zeros((50, 85), np.uint8)
        assert c.lib.lt_raw16_to_rgb(c._h, words.ctypes.data, 50, 68, 36, None, out.ctypes.data) == -1     # words are not packed rows
        conv = lambda layout, hh, ww, entries: c.lib.lt_raw_to_rgb_color(c._h, rows.ctypes.data, hh, ww, layout, lut10.ctypes.data, entries, None, None, out.ctypes.data)
        assert conv(36, 50, 68, 1024) == 0
        assert conv(36, 50, 66, 1024) == -1 and b"multiple of 4" in c.lib.lt_last_error()
        assert conv(36, 49, 68, 1024) == -1 and conv(36, 50, 68, 4096) == -1 and conv(52, 50, 67, 4096) == -1 and conv(40, 50, 68, 1024) == -1
        with pytest.raises(ValueError, match="input format only"):
            DeviceFrames.empty(1, (68, 50), "bayer10p_grbg")
        # a surface below the row's bytes, and one that is fine at any byte
        buf = DeviceBuffer(85 * 50 + 4)
        try:
            bad = DeviceFrames(np.zeros(1, _native.SURFACE_DTYPE), (68, 50), "bayer10p_grbg", owner=buf)
            bad.surfaces["plane"][0, 0], bad.surfaces["pitch"][0] = buf.ptr + 1, 84
            with pytest.raises(ValueError, match="below the row"):
                c.attach_device_frames(bad, first=0)
            bad.surfaces["pitch"][0] = 85                                                    # an odd address and an odd pitch are fine
            c.attach_device_frames(bad, first=0)
        finally:
            c.sync()
            buf.close()
    finally:
        c.close()
