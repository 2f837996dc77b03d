"""Raw sets on the device: one raw table, colour stage and shading map per slot of a context, per camera of a LaneTrackerGroup.

Kernel level (sizes A 64 x 48 and B 66 x 50 of front_matrix.py; packed RAW10 at 68 x 50, its width a multiple of 4): a context with three
raw sets that differ in table, matrix / curve, mesh and pedestals -- set 1 has no colour stage and set 2 no map, so a launch that mixes them
runs the union of the stages with a set's missing part as its identity -- and five slots with sets 0, 1, 2, 1, 0.  For every slot the
undistorted rows, the two planes and the shown camera frame equal, byte for byte, those of a ONE-set context that holds that set alone and
is given the same frames: the kernels the per-stage suites already hold to NumPy are the reference.  Everything is integers; every
comparison is np.array_equal.

Group level (1280 x 720): four cameras with three setups against solo trackers built with each camera's setup."""
import functools

import numpy as np
import pytest

import bayer_reference as RB
import front_matrix as FM
import test_gpu_bayer_wide as BW
import test_gpu_raw_color as GC
import test_gpu_raw_packed as RP
import test_gpu_raw_shading as GS
from lane_tracker_amd import _native, calib, utils
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

PATTERNS = list(RB.PATTERNS)
KINDS = ("8", "10", "12", "10p", "12p")
IDS = (0, 1, 2, 1, 0)
FIRST = 1                                # slots 1 .. 5: both parities of the interleaved pairs
WHAT = ("undistorted rows", "R plane", "Lab-b plane", "shown camera frame")


def bits_of(kind):
    return int(kind.rstrip("p"))


def size_of(kind, size):
    return (68, 50) if kind == "10p" and size == "B" else FM.SIZES[size]


def fmt_of(pattern, kind):
    bits = bits_of(kind)
    return pattern if bits == 8 else RP.names(pattern, bits)[0 if kind.endswith("p") else 1]


@functools.lru_cache(maxsize=None)
def samples(pattern, kind, wh, n=25):
    """n frames of samples of the kind's depth, (n, H, W); shared, never changed."""
    bits, (w, h) = bits_of(kind), wh
    out = np.random.default_rng(900 + 10 * bits + w + PATTERNS.index(pattern)).integers(0, 1 << bits, (n, h, w), dtype=np.uint16)
    out = out.astype(np.uint8) if bits == 8 else out
    out.setflags(write=False)
    return out


def frames_of(pattern, kind, wh, n=25):
    f = samples(pattern, kind, wh, n)
    return utils.pack_raw(f, fmt_of(pattern, kind)) if kind.endswith("p") else f


@functools.lru_cache(maxsize=None)
def setups(bits):
    """Three setups (table, (ccm, curve) or None, map or None): all parts unlike; 1 without a colour stage, 2 without a map."""
    if bits == 8:
        t = (GC.table8(), np.ascontiguousarray(GC.table8()[::-1, ::-1]), utils.raw_lut(16, 240, (1.9, 1, 1.6), "srgb"))
    else:
        t = tuple(x[1] for x in BW.tables(bits))
    st, mp = GC.stages(), GS.maps(bits)
    return ((t[0], st[3][1:], mp[1][1]), (t[1], None, mp[2][1]), (t[2], st[2][1:], None))


def apply(ctx, setup, raw_set=0):
    lut, stage, shading = setup
    ctx.set_raw_lut(lut, raw_set=raw_set)
    ctx.set_raw_color(*(stage if stage is not None else (None, None)), enable=stage is not None, raw_set=raw_set)
    ctx.set_raw_shading(shading, raw_set=raw_set)


def context(fmt, wh, capacity, calibrations=False):
    q = RP.calibration_sets(wh)
    c = _native.Context(wh, wh, q[0]["cam_matrix"], q[0]["dist_coeffs"], q[0]["M"], capacity=capacity)
    try:
        c.set_input_format(fmt)
        if calibrations:
            for s, k in enumerate(q[1:], 1):
                assert c.add_calibration(k["cam_matrix"], k["dist_coeffs"], k["M"]) == s
        c.overlay_configure(np.linalg.inv(q[0]["M"]))
    except BaseException:
        c.close()
        raise
    return c


def many_sets(fmt, wh, bits, capacity=8, calibrations=False):
    """A context whose raw sets 0, 1, 2 are setups(bits)."""
    c = context(fmt, wh, capacity, calibrations)
    try:
        apply(c, setups(bits)[0])
        for k in (1, 2):
            assert c.add_raw_set() == k
            apply(c, setups(bits)[k], raw_set=k)
        assert c.raw_set_count() == 3
    except BaseException:
        c.close()
        raise
    return c


def run(ctx, fmt, frames, first, source, raw_ids=None, cal_ids=None, shown=True):
    """Frames into slots first .., through the front end -> (undistorted rows, R plane, Lab-b plane, shown camera frames or None)."""
    n, (h, w) = len(frames), (ctx.img_h, ctx.img_w)
    if raw_ids is not None:
        ctx.set_slot_raw_sets(raw_ids, first=first)
    if cal_ids is not None:
        ctx.set_slot_calibrations(cal_ids, first=first)
    dev = None
    if source == "slots":
        ctx.upload_frames(frames, first=first)
    else:
        ctx.upload_frames(~frames, first=first)              # the slot's own staging frame is not the one to read
        dev = RP._surfaces_of(frames, fmt) if fmt not in RB.PATTERNS else BW._narrow_surfaces(frames, fmt)
    try:
        if dev is not None:
            ctx.attach_device_frames(dev, first=first)
        ctx.mask_run(n, first=first)
        form = ctx.last_raw_walk_form()
        if dev is not None and shown:
            ctx.device_frames_rest(n, first=first)
        out = (ctx.download_undistorted(n, first=first), ctx.download_plane(0, n, first=first), ctx.download_plane(1, n, first=first),
               BW._read_back(ctx, n, h, w, first) if shown else None)
        ctx.sync()
    finally:
        if dev is not None:
            dev.owner.close()
    return out, form


def references(fmt, wh, bits, frames, first, source, capacity=8, cal_ids=None, shown=True):
    """[s] -> what a one-set context with setups(bits)[s] alone makes of the frames."""
    out = []
    for s in range(3):
        c = context(fmt, wh, capacity, cal_ids is not None)
        try:
            apply(c, setups(bits)[s])
            assert c.raw_set_count() == 1
            got, form = run(c, fmt, frames, first, source, cal_ids=cal_ids, shown=shown)
            assert form == 1
            out.append(got)
        finally:
            c.close()
    return out


def compare(got, refs, ids, where):
    for i, s in enumerate(ids):
        for what, g, r in zip(WHAT, got, refs[s]):
            if g is not None:
                assert g[i].shape == r[i].shape and np.array_equal(g[i], r[i]), "%s: slot %d, raw set %d: %d bytes of the %s differ from a one-set context's" % (
                    where, i, s, int((g[i] != r[i]).sum()), what)


# ---- kernel level ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["A", "B"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_slot_of_a_mixed_run_is_its_own_sets_picture(pattern, kind, size):
    wh, bits, fmt = size_of(kind, size), bits_of(kind), fmt_of(pattern, kind)
    frames = frames_of(pattern, kind, wh)[:5]
    ctx = many_sets(fmt, wh, bits)
    try:
        for source in ("slots", "surfaces"):
            where = "%s %dx%d, %s" % ((fmt,) + wh + (source,))
            refs = references(fmt, wh, bits, frames, FIRST, source)
            assert len({r[0].tobytes() for r in refs}) == 3                      # the sets are not one picture
            got, form = run(ctx, fmt, frames, FIRST, source, raw_ids=IDS)
            assert form == 2, where
            assert list(ctx.slot_raw_sets(5, first=FIRST)) == list(IDS)
            compare(got, refs, IDS, where)
            # a uniform slice, on a set that is not 0: the one-set kernels, with that set's stages
            got, form = run(ctx, fmt, frames, FIRST, source, raw_ids=[2] * 5)
            assert form == 1, where
            compare(got, refs, [2] * 5, where + ", every slot on set 2")
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["8", "12", "10p"])
def test_a_long_run_crosses_the_slices(kind):
    pattern, wh, bits = "bayer_grbg", size_of(kind, "B"), bits_of(kind)
    fmt, n = fmt_of(pattern, kind), 25
    frames, ids = frames_of(pattern, kind, wh)[:n], [i % 3 for i in range(n)]
    ctx = many_sets(fmt, wh, bits, capacity=n + 2)
    try:
        ctx.set_streams(4)
        refs = references(fmt, wh, bits, frames, FIRST, "slots", capacity=n + 2, shown=False)
        got, form = run(ctx, fmt, frames, FIRST, "slots", raw_ids=ids, shown=False)
        assert form == 2
        compare(got, refs, ids, "%s, 25 slots over 4 slices" % fmt)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["8", "12p"])
def test_mixed_raw_sets_and_mixed_calibrations_in_one_run(kind):
    pattern, wh, bits = "bayer_gbrg", size_of(kind, "A"), bits_of(kind)
    fmt = fmt_of(pattern, kind)
    frames, cal_ids = frames_of(pattern, kind, wh)[5:10], FM.ids_pattern(5)
    ctx = many_sets(fmt, wh, bits, calibrations=True)
    try:
        for source in ("slots", "surfaces"):
            refs = references(fmt, wh, bits, frames, FIRST, source, cal_ids=cal_ids, shown=False)
            got, form = run(ctx, fmt, frames, FIRST, source, raw_ids=IDS, cal_ids=cal_ids, shown=False)
            assert form == 2
            compare(got, refs, IDS, "%s, %s, calibration sets %r" % (fmt, source, cal_ids))
            # one calibration set, mixed raw sets; and mixed calibration sets over one raw set
            refs1 = references(fmt, wh, bits, frames, FIRST, source, cal_ids=[3] * 5, shown=False)
            got, form = run(ctx, fmt, frames, FIRST, source, raw_ids=IDS, cal_ids=[3] * 5, shown=False)
            assert form == 2
            compare(got, refs1, IDS, "%s, %s, calibration set 3" % (fmt, source))
            got, form = run(ctx, fmt, frames, FIRST, source, raw_ids=[1] * 5, cal_ids=cal_ids, shown=False)
            assert form == 1
            compare(got, refs, [1] * 5, "%s, %s, raw set 1" % (fmt, source))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["8", "12"])
def test_changing_one_set_changes_its_slots_and_no_other(kind):
    pattern, wh, bits = "bayer_rggb", size_of(kind, "A"), bits_of(kind)
    fmt = fmt_of(pattern, kind)
    frames = frames_of(pattern, kind, wh)[:5]
    other = np.ascontiguousarray(setups(bits)[1][0][:, ::-1])
    ctx = many_sets(fmt, wh, bits)
    try:
        before, form = run(ctx, fmt, frames, FIRST, "slots", raw_ids=IDS)
        assert form == 2
        ctx.set_raw_lut(other, raw_set=1)
        assert np.array_equal(ctx.raw_lut(raw_set=1), other) and np.array_equal(ctx.raw_lut(), setups(bits)[0][0])
        # only the slots of set 1 are stale: a re-run recomputes their planes and leaves the others' as they are
        ctx.mask_run(5, first=FIRST, reuse_front=True)
        assert ctx.last_raw_walk_form() == 2                   # (the slice holds stale slots: its front end runs)
        after, _ = run(ctx, fmt, frames, FIRST, "slots", raw_ids=IDS)
        one = context(fmt, wh, 8)
        try:
            apply(one, (other,) + setups(bits)[1][1:])
            want, _ = run(one, fmt, frames, FIRST, "slots")
        finally:
            one.close()
        for i, s in enumerate(IDS):
            for what, b, a, w_ in zip(WHAT, before, after, want):
                if s == 1:
                    assert np.array_equal(a[i], w_[i]) and not np.array_equal(a[i], b[i]), (what, i)
                else:
                    assert np.array_equal(a[i], b[i]), (what, i)
        # staleness as the context reports it: after a change of set 1, a re-run over slots of sets 0 and 2 alone runs no front end
        ctx.set_raw_lut(setups(bits)[1][0], raw_set=1)
        ctx.mask_run(1, first=FIRST, reuse_front=True)         # slot 1: set 0
        assert ctx.last_raw_walk_form() == 0
        ctx.mask_run(1, first=FIRST + 2, reuse_front=True)     # slot 3: set 2
        assert ctx.last_raw_walk_form() == 0
        ctx.mask_run(1, first=FIRST + 1, reuse_front=True)     # slot 2: set 1
        assert ctx.last_raw_walk_form() == 1
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["8", "12", "10p"])
def test_statistics_read_each_slots_own_map(kind):
    pattern, wh, bits = "bayer_bggr", size_of(kind, "B"), bits_of(kind)
    fmt = fmt_of(pattern, kind)
    frames, raw = frames_of(pattern, kind, wh)[:5], samples(pattern, kind, wh)[:5]
    ctx = many_sets(fmt, wh, bits)
    try:
        ctx.set_slot_raw_sets(IDS, first=FIRST)
        ctx.upload_frames(frames, first=FIRST)
        got = ctx.raw_stats(5, first=FIRST, grid=(3, 4))
        for i, s in enumerate(IDS):
            want = utils.raw_stats(raw[i], _native.unpacked_format(fmt), grid=(3, 4), rows=got.rows, shading=setups(bits)[s][2])
            assert np.array_equal(got.hist[i], want.hist) and np.array_equal(got.zone_count[i], want.zone_count) and \
                np.array_equal(got.zone_sum[i], want.zone_sum), (i, s)
    finally:
        ctx.close()


def test_refusals_leave_the_context_usable():
    pattern, wh = "bayer_rggb", FM.SIZES["A"]
    fmt = fmt_of(pattern, "12")
    frames = frames_of(pattern, "12", wh)[:5]
    ctx = many_sets(fmt, wh, 12)
    rgb = _native.Context(wh, wh, np.eye(3), np.zeros(5), np.eye(3), capacity=2)
    try:
        refs = references(fmt, wh, 12, frames, FIRST, "slots", shown=False)
        with pytest.raises(ValueError, match="raw set 3 out of range"):
            ctx.set_slot_raw_sets([0, 3], first=FIRST)
        with pytest.raises(ValueError, match="raw set 7 out of range"):
            ctx.set_raw_color(None, None, raw_set=7)
        wrong = np.zeros((4, 1024), np.uint8)
        assert ctx.lib.lt_set_raw_lut_of(ctx._h, 1, wrong.ctypes.data, 1024) == -1 and b"4096" in ctx.lib.lt_last_error()
        assert ctx.lib.lt_set_raw_lut_of(rgb._h, 0, wrong.ctypes.data, 1024) == -5            # LT_ERR_STATE: not a raw context
        i = _native.C.c_int(0)
        assert rgb.lib.lt_add_raw_set(rgb._h, _native.C.byref(i)) == -5 and rgb.raw_set_count() == 1
        assert rgb.lib.lt_set_raw_shading_of(rgb._h, 0, None, 0, 0, None, 0) == -5
        assert ctx.raw_set_count() == 3
        got, form = run(ctx, fmt, frames, FIRST, "slots", raw_ids=IDS, shown=False)
        assert form == 2
        compare(got, refs, IDS, "after the refusals")
    finally:
        ctx.close()
        rgb.close()


# ---- group level ---------------------------------------------------------------------------------------------------------------------------
def _camera_setups(pattern, bits):
    """(frames, the four cameras' setups as raw_setups takes them -- three distinct: 0 and 3 are the group's own --, a further table)."""
    raw, one, two = BW._scenes(pattern, bits) if bits > 8 else (None, None, None)
    if bits == 8:
        r16, one16, two16 = BW._scenes(pattern, 10)
        raw = (r16 >> 2).astype(np.uint8)
        one, two = utils.raw_lut(16, 16 + 127, (1.05, 1, 0.95), 1.1), utils.raw_lut(16, 16 + 127, (1, 1, 1.02), 1.0)
    m, t = utils.raw_ccm([[1.05, -0.05, 0.0], [0.0, 1.0, 0.0], [0.0, -0.05, 1.05]]), utils.raw_curve(1.0)
    sh = GS.vignette(bits, 0.2)
    own = dict(raw_lut=one, raw_ccm=None, raw_curve=None, raw_shading=None)
    cams = [None, dict(raw_shading=sh), dict(raw_lut=two, raw_ccm=m, raw_curve=t), {}]
    full = [dict(own, **(c or {})) for c in cams]
    third = utils.raw_lut(*((16, 16 + 127) if bits == 8 else ((1 << bits) // 16, (1 << bits) // 16 + 255 * (1 << (bits - 9)))), (1.02, 1, 1.0), 1.05, bits=bits)
    return raw, own, cams, full, third


@pytest.mark.parametrize("pattern,bits", [("bayer_grbg", 8), ("bayer_gbrg", 12)])
def test_a_group_of_unlike_cameras_equals_solo_trackers(pattern, bits):
    cal = calib.reference_calibration()
    fmt = pattern if bits == 8 else BW.wide_name(pattern, bits)
    raw, own, cams, full, third = _camera_setups(pattern, bits)
    g = LaneTrackerGroup(4, **cal, pixel_format=fmt, raw_setups=cams, **own)
    solos = [LaneTracker(**cal, pixel_format=fmt, **s) for s in full]
    try:
        assert g.raw_set_count() == 3 and g._raw_ids[0] == g._raw_ids[3] == 0
        for i, s in enumerate(full):
            t = g.trackers[i]
            assert np.array_equal(t.raw_lut, s["raw_lut"]) and (t.raw_ccm is None) == (s["raw_ccm"] is None) and (t.raw_shading is None) == (s["raw_shading"] is None)

        def tick(k, skip=None):
            fr = [None if i == skip else raw[(k + i) % len(raw)] for i in range(4)]
            outs = g.process(fr)
            for i in range(4):
                if i == skip:
                    assert outs[i] is None
                    continue
                assert np.array_equal(outs[i], solos[i].process(fr[i])), (k, i)
                assert BW._get_state(g.trackers[i]) == BW._get_state(solos[i]), (k, i)
            return fr

        tick(0)
        assert g._ctx.last_raw_walk_form() == 2
        tick(1, skip=1)
        # camera 2's white balance moves between ticks; the others are unmoved
        g.set_raw_lut(third, stream=2)
        solos[2].set_raw_lut(third)
        assert g.raw_set_count() == 3 and np.array_equal(g.trackers[2].raw_lut, third) and np.array_equal(g.trackers[0].raw_lut, own["raw_lut"])
        tick(2)
        # statistics of camera 1, behind its map, leave every state as it is
        before = [BW._get_state(t) for t in g.trackers]
        got = g.raw_stats(raw[:2], stream=1, grid=(4, 4))
        want = utils.raw_stats(raw[:2], fmt, grid=(4, 4), rows=got.rows, shading=full[1]["raw_shading"])
        assert np.array_equal(got.hist, want.hist) and np.array_equal(got.zone_sum, want.zone_sum) and np.array_equal(got.zone_count, want.zone_count)
        assert [BW._get_state(t) for t in g.trackers] == before
        tick(3)
        assert solos[0].success >= 3
        with pytest.raises(RuntimeError):
            g.trackers[1].set_raw_lut(third)
    finally:
        g.close()
        for s in solos:
            s.close()


def test_a_group_without_raw_setups_runs_the_one_set_kernels():
    cal = calib.reference_calibration()
    pattern, bits = "bayer_rggb", 12
    fmt = BW.wide_name(pattern, bits)
    raw, one, _ = BW._scenes(pattern, bits)
    g = LaneTrackerGroup(2, **cal, pixel_format=fmt, raw_lut=one)
    try:
        g.process([raw[0], raw[1]], annotate=False)
        assert g.raw_set_count() == 1 and g._ctx.raw_set_count() == 1 and g._ctx.last_raw_walk_form() == 1
    finally:
        g.close()
