"""Raw Bayer statistics on the device (lt_raw_stats, k_raw_stats.hip): `Context.raw_stats` equals `utils.raw_stats`, the NumPy definition,
EXACTLY -- histograms, zone counts and zone sums are integers, so any order the device adds in gives the same bits -- over every format,
source, slot range, grid, rectangle, pair of bounds, with and without a shading map; the call disturbs nothing; what it refuses; and the
tracker's method, on host frames and frames in device memory.

Sizes: 64 x 48 for all; the odd row bytes 68 x 50 (RAW10: 85 bytes a row) and 66 x 50 (RAW12: 99; bytes: 66; words: 132).  Frames: the pool
of test_gpu_raw_packed.py at the format's bits -- all zero and all maximum (every thread hits one bin), only low bits, only high bytes, the
x % 4, y % 2 frame, random ones -- and for 16-bit words one more with random garbage above the sample's bits; two sets of five, A = the five
special frames and B = random ones (with the garbage frame), each at first = 1 and at first = 2 of a context of 8 slots.  Surfaces: padded --
pitch = row bytes + 3 and the plane at byte 1 of its block; 16-bit words, which the library takes at even addresses and pitches only, pitch
= row bytes + 6 at byte 2 -- and dense, the last row ending on the block's last byte, read with a rectangle that holds the bottom-right cell
among others.  A grid side of 64 fits none of these sizes: test_a_grid_side_of_64 runs it on frames of 136 x 48."""
import ctypes as C
import functools

import numpy as np
import pytest

import bayer_reference as RB
import test_gpu_bayer_wide as BW
import test_gpu_raw_packed as RP
import test_gpu_raw_shading as GS
from lane_tracker_amd import _native, calib, synth, utils
from lane_tracker_amd.device import DeviceFrames
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

PATTERNS = list(RB.PATTERNS)
KINDS = ("8", "10", "12", "10p", "12p")
N, CAPACITY = 5, 8
SIZES = {"8": ((64, 48), (66, 50)), "10": ((64, 48), (66, 50)), "12": ((64, 48), (66, 50)), "10p": ((64, 48), (68, 50)), "12p": ((64, 48), (66, 50))}
SOURCES = ("upload", "rows", "surfaces", "surfaces to the last byte")


def _context(fmt, wh, capacity=CAPACITY):
    """A context of one calibration whose path reads a narrow run of camera rows (test_gpu_raw_packed.calibration_sets: set 2, source rows
    [15, 40) of 48 / [15, 41) of 50): the default rectangle is not the whole frame, and its first row has to be rounded."""
    q = RP.calibration_sets(wh)[2]
    c = _native.Context(wh, wh, q["cam_matrix"], q["dist_coeffs"], q["M"], capacity=capacity)
    try:
        c.set_input_format(fmt)
        c.set_streams(1)
        r0, r1 = c.input_rows()
        assert 0 < r0 and r1 < wh[1] and r1 - r0 >= 4, (r0, r1)
    except BaseException:
        c.close()
        raise
    return c


def fmt_of(pattern, kind):
    return pattern if kind == "8" else "bayer%s_%s" % (kind, pattern[6:])


def bits_of(kind):
    return int(kind.rstrip("p"))


@functools.lru_cache(maxsize=None)
def frame_sets(kind, wh):
    """-> (A, B): five frames each in the format's own form, from test_gpu_raw_packed.pool."""
    bits = bits_of(kind)
    pool = RP.pool(bits, wh)
    a, b = pool[:5].copy(), pool[5:10].copy()
    if kind == "8":
        a, b = a.astype(np.uint8), b.astype(np.uint8)
    elif kind.endswith("p"):
        a, b = utils.pack_raw(a, kind), utils.pack_raw(b, kind)
    else:
        rng = np.random.default_rng(bits)
        b[4] |= rng.integers(1, 1 << (16 - bits), b.shape[1:], dtype=np.uint16) << bits       # garbage above the sample: ignored, as everywhere
        assert (b[4] >> bits).all()
    a.setflags(write=False), b.setflags(write=False)
    return a, b


def surfaces_of(frames, fmt, padded):
    if fmt in _native.BAYER_PACKED_FORMATS:
        return RP._packed_surfaces(frames, fmt, padded)
    if fmt in _native.BAYER_WIDE_FORMATS:
        return BW._wide_surfaces(frames, fmt, padded)
    kw = dict(pitch=frames.shape[-1] + 3, offset=1) if padded else {}
    block, surf, size, single = RP.pack_host_frames(frames, fmt, fill=RP.FM.FILL, **kw)
    assert block.nbytes == (1 if padded else 0) + int(surf["pitch"][0]) * (frames.shape[0] * frames.shape[1] - 1) + frames.shape[-1]
    buf = RP.DeviceBuffer(block.nbytes).copy_from_host(block)
    surf["plane"][:, :1] += np.uint64(buf.ptr)
    return DeviceFrames(surf, size, fmt, owner=buf, single=single)


class Source:
    """Frames F in slots [first, first + N) of `ctx`, by one of the four sources; closes what it allocated."""

    def __init__(self, ctx, fmt, frames, first, source):
        self.dev = None
        if source == "upload":
            ctx.upload_frames(frames, first=first)
        elif source == "rows":
            ctx.upload_frames(~frames, first=first)              # what the slots held before: not what is measured
            ctx.upload_frame_rows(frames, first=first)
        else:
            ctx.upload_frames(~frames, first=first)              # the slots' own staging frames are not the ones to read
            self.dev = surfaces_of(frames, fmt, padded=source == "surfaces")
            ctx.attach_device_frames(self.dev, first=first)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.dev is not None:
            self.dev.owner.close()


def rectangles(ctx, wh):
    """name -> (rows, cols) as the call takes them: the default, the whole frame, a corner of 2 x 2 cells (the bottom-right one)."""
    w, h = wh
    return {"default": (None, None), "whole": ((0, h), (0, w)), "corner": ((h - 4, h), (w - 4, w))}


def assert_equal(got, want, where):
    assert got.rows == want.rows and got.cols == want.cols, (where, got.rows, got.cols, want.rows, want.cols)
    for name, g, w in zip(("hist", "zone_count", "zone_sum"), got[:3], want[:3]):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), "%s: %s differs at %d of %d places" % (where, name, int((g != w).sum()), g.size)


@pytest.mark.parametrize("size", [0, 1], ids=["64x48", "odd row bytes"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_device_statistics_equal_the_numpy_definition(pattern, kind, size):
    fmt, wh, bits = fmt_of(pattern, kind), SIZES[kind][size], bits_of(kind)
    smax = (1 << bits) - 1
    sets = frame_sets(kind, wh)
    ctx = _context(fmt, wh)
    try:
        d0, d1 = _native.default_stats_rows(ctx.input_rows())
        assert 0 <= d0 < d1 <= wh[1] and d0 % 2 == d1 % 2 == 0
        rects = rectangles(ctx, wh)
        want = {}                                              # the definition, once per (shading, set, rectangle, grid, bounds)
        calls = 0
        for shading in (None, GS.maps(bits)[2 + PATTERNS.index(pattern) % 2][1]):      # none; the random map or the vignette
            ctx.set_raw_shading(shading)
            for source in SOURCES:
                for first in (1, 2):
                    for si, frames in enumerate(sets):
                        with Source(ctx, fmt, frames, first, source):
                            for rname, (rows, cols) in rects.items():
                                if source == "rows" and rname != "default":
                                    continue                   # (only the rows came: the library refuses other rows, test_refusals)
                                r = (d0, d1) if rows is None else rows
                                c = (0, wh[0]) if cols is None else cols
                                ncy, ncx = (r[1] - r[0]) // 2, (c[1] - c[0]) // 2
                                for grid in dict.fromkeys([(1, 1), (min(3, ncy), min(5, ncx)), (ncy, ncx)]):
                                    for lo, hi in ((None, None), (1, smax - 1)):
                                        key = (id(shading), si, rname, grid, lo)
                                        if key not in want:
                                            want[key] = utils.raw_stats(frames, fmt, grid, r, c, lo, hi, shading)
                                        got = ctx.raw_stats(N, first, grid, rows, cols, lo, hi)
                                        calls += 1
                                        assert_equal(got, want[key], "%s %dx%d, %s, slots [%d, %d), set %s, %s rectangle, grid %r, lo %r, map %s" % (
                                            fmt, wh[0], wh[1], source, first, first + N, "AB"[si], rname, grid, lo, shading is not None))
        # what the cases above rest on: the flat frames put every site of a phase into one bin, and lo = 1, hi = smax - 1 leaves them no cell
        flat = want[(id(None), 0, "whole", (1, 1), 1)]
        assert flat.zone_count[:2].sum() == 0 and flat.zone_sum[:2].sum() == 0 and (flat.hist[0, :, 0] == wh[0] * wh[1] // 4).all()
        assert (flat.hist[1, :, smax] == wh[0] * wh[1] // 4).all() and flat.zone_count[4].sum() > 0
        assert calls == 2 * (3 * 2 * 2 * (3 + 3 + 2) * 2 + 1 * 2 * 2 * 3 * 2)      # every listed combination ran
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_grid_side_of_64(kind):
    """64 zones on an axis, and 24 x 64 zones of one cell row each -- the most zone rows a band of cell rows can touch --: frames of 136 x 48
    in every sample form, from staging and from both kinds of surfaces, with and without a map, whole-frame and default rectangles."""
    wh, fmt, bits = (136, 48), fmt_of("bayer_gbrg", kind), bits_of(kind)
    frames = frame_sets(kind, wh)[1]
    ctx = _context(fmt, wh)
    try:
        d0, d1 = _native.default_stats_rows(ctx.input_rows())
        for shading in (None, GS.maps(bits)[2][1]):
            ctx.set_raw_shading(shading)
            for source in ("upload", "surfaces", "surfaces to the last byte"):
                with Source(ctx, fmt, frames, 2, source):
                    for grid, rows in (((1, 64), None), ((24, 64), (0, 48)), ((3, 64), (0, 48)), ((min(5, (d1 - d0) // 2), 64), None)):
                        want = utils.raw_stats(frames, fmt, grid, (d0, d1) if rows is None else rows, shading=shading)
                        assert_equal(ctx.raw_stats(N, 2, grid, rows), want, "%s %s grid %r rows %r map %s" % (fmt, source, grid, rows, shading is not None))
        with pytest.raises(ValueError):
            ctx.raw_stats(N, 2, (1, 65), (0, 48))
    finally:
        ctx.close()


@pytest.mark.parametrize("pattern,kind", [("bayer_grbg", "8"), ("bayer_rggb", "12"), ("bayer_gbrg", "10p")])
def test_a_range_of_attached_and_uploaded_slots(pattern, kind):
    """One call over slots that take turns between their staging frames and attached surfaces: uploaded 1 .. 5 with slots 2 .. 3 attached to
    other frames, then slots 1 and 5 attached as well -- every slot's statistics are those of what IT holds, in the order of the slots."""
    fmt, wh = fmt_of(pattern, kind), SIZES[kind][1]
    up, other = frame_sets(kind, wh)
    ctx = _context(fmt, wh)
    try:
        ctx.upload_frames(up, first=1)
        devs = [surfaces_of(other[1:3], fmt, padded=True)]
        try:
            ctx.attach_device_frames(devs[0], first=2)
            held = np.stack([up[0], other[1], other[2], up[3], up[4]])
            for grid, rows in (((2, 3), None), ((1, 1), (0, wh[1])), ((2, 2), (wh[1] - 4, wh[1]))):
                want = utils.raw_stats(held, fmt, grid, _native.default_stats_rows(ctx.input_rows()) if rows is None else rows)
                assert_equal(ctx.raw_stats(N, 1, grid, rows), want, "%s staging, surfaces x 2, staging x 2, grid %r" % (fmt, grid))
                part = ctx.raw_stats(3, 2, grid, rows)                     # a range that starts on an attached slot
                assert all(np.array_equal(g, w[1:4]) for g, w in zip(part[:3], want[:3])), (fmt, grid)
            devs.append(surfaces_of(other[:1], fmt, padded=False))
            devs.append(surfaces_of(other[4:], fmt, padded=False))
            ctx.attach_device_frames(devs[1], first=1)
            ctx.attach_device_frames(devs[2], first=5)
            ctx.upload_frames(up[1:2], first=2)                            # an upload detaches: slot 2 is its staging frame again
            held = np.stack([other[0], up[1], other[2], up[3], other[4]])
            want = utils.raw_stats(held, fmt, (3, 4), (0, wh[1]))
            assert_equal(ctx.raw_stats(N, 1, (3, 4), (0, wh[1])), want, "%s surfaces and staging in turns" % fmt)
        finally:
            for d in devs:
                d.owner.close()
    finally:
        ctx.close()


# ---- the call disturbs nothing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,kind", [("bayer_rggb", "8"), ("bayer_grbg", "12"), ("bayer_bggr", "10p")])
def test_statistics_disturb_nothing(pattern, kind):
    fmt, wh = fmt_of(pattern, kind), SIZES[kind][1]
    frames = frame_sets(kind, wh)[1]
    shading = GS.maps(bits_of(kind))[3][1]
    a, b = _context(fmt, wh), _context(fmt, wh)
    try:
        for source in SOURCES:
            outs = []
            for ctx, measured in ((a, True), (b, False)):
                ctx.set_raw_shading(shading)
                with Source(ctx, fmt, frames, 1, source):
                    if measured:
                        ctx.raw_stats(N, 1, (1, 5))
                        if source != "rows":
                            ctx.raw_stats(N, 1, (2, 2), (0, wh[1]), (0, wh[0]), 1)
                    ctx.mask_run(N, first=1)
                    if measured:
                        ctx.raw_stats(N, 1, (1, 1))            # (between the chain and the downloads too)
                    outs.append((ctx.download_undistorted(N, first=1), ctx.download_plane(0, N, first=1), ctx.download_plane(1, N, first=1),
                                 ctx.download_masks(N, first=1), ctx.last_threshold_path(), ctx.last_open_form()))
                    ctx.sync()
            for x, y in zip(*outs):
                assert np.array_equal(x, y), (fmt, source)
    finally:
        a.close()
        b.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def _raw_call(ctx, first, n, p, bins=256, zones=1):
    hist, count, total, rect = np.full((max(n, 1), 4, bins), 7, np.uint32), np.full((max(n, 1), zones), 7, np.uint32), np.full((max(n, 1), zones, 4), 7, np.uint64), np.full(4, 7, np.int32)
    rc = ctx.lib.lt_raw_stats(ctx._h, first, n, None if p is None else C.byref(p), hist.ctypes.data, count.ctypes.data, total.ctypes.data, rect.ctypes.data)
    return rc, hist, count, total, rect


def _params(rows=(0, 0), cols=(0, 0), grid=(1, 1), lo=(0, 0, 0, 0), hi=(255, 255, 255, 255)):
    return _native.RawStatsParams(rows[0], rows[1], cols[0], cols[1], grid[0], grid[1], (C.c_int32 * 4)(*lo), (C.c_int32 * 4)(*hi))


def test_refusals():
    LT_ERR_INVALID, LT_ERR_STATE = -1, -5
    wh = (64, 48)
    cal = RP.calibration_sets(wh)[0]
    for fmt, tail in (("rgb", (48, 64, 3)), ("nv12", (72, 64))):
        c = _native.Context(wh, wh, cal["cam_matrix"], cal["dist_coeffs"], cal["M"], capacity=2)
        try:
            c.set_input_format(fmt)
            c.upload_frames(np.zeros((1,) + tail, np.uint8))
            rc, hist, _, _, rect = _raw_call(c, 0, 1, _params())
            assert rc == LT_ERR_STATE and b"raw Bayer" in c.lib.lt_last_error() and (hist == 7).all() and (rect == 7).all(), fmt
            with pytest.raises(ValueError, match="raw"):
                c.raw_stats(1)
        finally:
            c.close()
    fmt = "bayer_grbg"
    frames = frame_sets("8", wh)[1]
    ctx = _context(fmt, wh)
    try:
        d = _native.default_stats_rows(ctx.input_rows())
        good = lambda: assert_equal(ctx.raw_stats(N, 1, (2, 3)), utils.raw_stats(frames, fmt, (2, 3), d), "after a refusal")
        # a slot that was never complete: only the path's rows came
        ctx.upload_frame_rows(frames, first=1)
        good()
        for rows in ((0, 48), (d[0], 48) if d[1] < 48 else (0, d[1]), (0, 2)):
            rc, hist, _, _, rect = _raw_call(ctx, 1, N, _params(rows, (0, 64)))
            assert rc == LT_ERR_STATE and b"slot 1" in ctx.lib.lt_last_error() and (hist == 7).all() and (rect == 7).all(), rows
            with pytest.raises(RuntimeError):
                ctx.raw_stats(N, 1, (1, 1), rows)
            good()
        # ... and one whole frame among them does not help the others
        ctx.upload_frames(frames[:1], first=1)
        assert _raw_call(ctx, 1, N, _params((0, 48)))[0] == LT_ERR_STATE and b"slot 2" in ctx.lib.lt_last_error()
        assert _raw_call(ctx, 1, 1, _params((0, 48)))[0] == 0
        ctx.upload_frames(frames, first=1)
        good()
        # the argument errors, past the Python checks
        bad = [None, _params((1, 48)), _params((0, 47)), _params((0, 50)), _params((-2, 48)), _params((20, 20)), _params((30, 20)), _params(cols=(1, 64)),
               _params(cols=(0, 63)), _params(cols=(0, 66)), _params(cols=(-2, 64)), _params(cols=(8, 8)), _params(grid=(0, 1)), _params(grid=(1, 0)),
               _params(grid=(65, 1)), _params(grid=(1, 65)), _params((0, 48), grid=(25, 1)), _params((0, 48), grid=(1, 33)), _params((0, 4), (0, 4), (3, 1)),
               _params(lo=(0, 0, -1, 0)), _params(lo=(256, 0, 0, 0)), _params(hi=(255, 256, 255, 255)), _params(hi=(255, 255, 255, -1))]
        for p in bad:
            rc, hist, count, total, rect = _raw_call(ctx, 1, N, p)
            assert rc == LT_ERR_INVALID and (hist == 7).all() and (count == 7).all() and (total == 7).all() and (rect == 7).all(), p and [getattr(p, f[0]) for f in p._fields_[:6]]
            good()
        for first, n in ((-1, 2), (0, -1), (4, N), (CAPACITY, 1), (0, CAPACITY + 1)):
            assert _raw_call(ctx, first, n, _params())[0] == LT_ERR_INVALID, (first, n)
        good()
        # n == 0 is fine and touches nothing but the rectangle; lo > hi is legal: no valid cell
        rc, hist, _, _, rect = _raw_call(ctx, 3, 0, _params())
        assert rc == 0 and (hist == 7).all() and rect.tolist() == [d[0], d[1], 0, 64]
        assert _raw_call(ctx, CAPACITY, 0, _params())[0] == 0
        none = ctx.raw_stats(N, 1, (2, 2), lo=200, hi=100)
        assert not none.zone_count.any() and not none.zone_sum.any() and int(none.hist.sum()) == N * (d[1] - d[0]) * 64
        # any output may be left out
        want = utils.raw_stats(frames, fmt, (1, 1), d)
        hist, total = np.zeros((N, 4, 256), np.uint32), np.zeros((N, 1, 1, 4), np.uint64)
        assert ctx.lib.lt_raw_stats(ctx._h, 1, N, C.byref(_params()), hist.ctypes.data, None, None, None) == 0 and np.array_equal(hist, want.hist)
        assert ctx.lib.lt_raw_stats(ctx._h, 1, N, C.byref(_params()), None, None, total.ctypes.data, None) == 0 and np.array_equal(total, want.zone_sum)
        assert ctx.lib.lt_raw_stats(ctx._h, 1, N, C.byref(_params()), None, None, None, None) == 0
        good()
    finally:
        ctx.close()


# ---- the tracker --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scenes(pattern, kind):
    """Three rendered scenes as the sensor delivers them in this format, a pedestal of a sixteenth of full scale under half-scale samples."""
    bits = bits_of(kind)
    r = synth.SceneRenderer()
    m = RB.rgb_to_bayer(np.stack([r.render(s)[0] for s in range(3)]), pattern).astype(np.uint16)
    top = 1 << bits
    raw = (m << (bits - 8)) // 2 + top // 16
    raw = raw.astype(np.uint8) if kind == "8" else utils.pack_raw(raw, kind) if kind.endswith("p") else raw
    raw.setflags(write=False)
    return raw


@pytest.mark.parametrize("pattern,kind", [("bayer_rggb", "8"), ("bayer_grbg", "12"), ("bayer_bggr", "10p")])
def test_tracker_raw_stats_on_host_and_device_frames(pattern, kind):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    fmt, bits = fmt_of(pattern, kind), bits_of(kind)
    black, white = (1 << bits) // 16, (1 << bits) // 16 + (1 << bits) // 2
    frames = _scenes(pattern, kind)
    shading = GS.vignette(bits, 0.5)
    t, twin = LaneTracker(**cal, pixel_format=fmt, raw_shading=shading), LaneTracker(**cal, pixel_format=fmt, raw_shading=shading)
    dev = DeviceFrames.from_host(frames, fmt)
    order = [2, 0, 1, 1, 2]
    dev5 = DeviceFrames.from_host(np.ascontiguousarray(frames[order]), fmt)
    try:
        assert np.array_equal(t.raw_shading.mesh, shading.mesh)
        d = _native.default_stats_rows(t._ctx.input_rows())
        before = t.get_state()
        want = utils.raw_stats(frames, fmt, rows=d, shading=t.raw_shading)
        host, device = t.raw_stats(frames), t.raw_stats(dev)
        assert_equal(host, want, "%s host frames" % fmt)
        assert_equal(device, want, "%s device frames" % fmt)
        assert utils.awb_gains(host, black) == utils.awb_gains(device, black) == utils.awb_gains(want, black)
        # the tracker's context holds two slots: the three frames above went in two pieces; five device frames go in three, attached piece
        # by piece, and come back in the frames' order
        assert t._ctx.capacity == 2
        five = t.raw_stats(dev5, grid=(2, 3))
        assert_equal(five, utils.raw_stats(frames[order], fmt, (2, 3), d, shading=shading), "%s five device frames in pieces of two" % fmt)
        assert t._ctx.capacity == 2 and t._rows_keepalive is dev5
        one = t.raw_stats(frames[2], grid=(4, 4), rows=(0, H), lo=black, hi=white)          # rows outside the default run: the whole frame goes up
        assert_equal(one, utils.raw_stats(frames[2], fmt, (4, 4), (0, H), None, black, white, shading), "%s one whole frame" % fmt)
        assert_equal(t.raw_stats(dev[1], rows=(0, H)), utils.raw_stats(frames[1], fmt, rows=(0, H), shading=shading), "%s one device frame" % fmt)
        assert t.get_state() == before and t.counter == 0
        with pytest.raises(ValueError):
            t.raw_stats(frames[:, :-2])
        # what follows is what a tracker that never asked computes
        for k in range(2):
            oa, ob = t.process(frames[k]), twin.process(frames[k])
            assert np.array_equal(oa, ob), (fmt, k)
            assert t._ctx.download_records(1).tobytes() == twin._ctx.download_records(1).tobytes()
        BW._same(t, twin)
        # the loop closed: the measured gains into the table, between frames
        s = t.raw_stats(frames[:2], lo=black, hi=white)
        lut = utils.raw_lut(black, white, utils.awb_gains(s, black), 1.0, bits)
        for x in (t, twin):
            x.set_raw_lut(lut)
        assert np.array_equal(t.process(frames[2]), twin.process(frames[2]))
        BW._same(t, twin)
    finally:
        t.close()
        twin.close()
        dev.owner.close()
        dev5.owner.close()
