"""Annotated frames drawn on their way into device sinks (lt_overlay_run_to_surfaces) and the table-per-slot forms of the presentation
kernels (a range of slots that mixes calibration sets in one launch, lt_last_overlay_launches).  Everything is bit for bit against
the existing routes: overlay_run + overlay_text + download_overlay on a twin context (and utils.rgb_to_yuv of that for 4:2:0 sinks),
or the same slots computed set by set on one-set contexts.  The sink blocks end on the last byte of the last plane and carry FILL
between and around the rows, which must stay."""
import itertools

import numpy as np
import pytest

from lane_tracker_amd import _native, utils
from lane_tracker_amd.device import DeviceFrames
from test_gpu_inplace_device import FONT, LAYOUTS, TEXT_KW, TEXTS, _annotated, _noise, _polygons, _refused, _small_ctx, _Surfaces

pytestmark = pytest.mark.gpu

SIZE = (64, 48)
# the inverse warps of three calibration sets: identity, a shift by (3, -2), a mild perspective
MINV = [np.eye(3), np.array([[1.0, 0.0, 3.0], [0.0, 1.0, -2.0], [0.0, 0.0, 1.0]]),
        np.array([[1.0, 0.05, -1.0], [0.02, 1.0, 0.5], [0.0, 0.0008, 1.0]])]


def _sink_shape(n, h, w, layout):
    return (n, h, w, 3) if layout == "rgb" else (n, h * 3 // 2, w)


def _sink(n, h, w, layout, extra=0, offset=0):
    """n surfaces of zeros in a block with FILL between and around the rows."""
    return _Surfaces(np.zeros(_sink_shape(n, h, w, layout), np.uint8), layout, extra, offset)


def _in_layout(annotated, layout, matrix="bt601"):
    return annotated if layout == "rgb" else np.stack([utils.rgb_to_yuv(f, layout, matrix) for f in annotated])


def _pick(turn, n, polys):
    return [polys[(turn + i) % 3] for i in range(n)], [TEXTS[(turn + 2 * i) % 3] for i in range(n)]


# ---- 1. the kernels at their edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 48), (66, 48), (62, 46)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernels_at_their_edges(layout, size):
    w, h = size
    a, b = _small_ctx(size, "rgb", 4), _small_ctx(size, "rgb", 4)
    polys = _polygons(w, h)
    try:
        assert b.last_overlay_launches() == -1
        for n in (1, 3):
            frames = _noise(n, h, w, "rgb", seed=100 * n + w)
            want_of = {}                                                    # (the polygons and texts repeat every three turns)
            for turn, (extra, offset) in enumerate(itertools.product((0, 1, 37), range(4))):
                first = turn % 2                                            # (the launch's first slot is not always slot 0)
                ps, ts = _pick(turn, n, polys)
                if turn % 3 not in want_of:
                    annotated = _annotated(a, frames, ps, ts)
                    changed = (annotated != frames).any(axis=3)
                    if any(len(p[0]) for p in ps):
                        assert changed[:, 19:].any(), "no lane pixel changed below the text"
                    assert changed[:, 3:19].any(), "no pixel changed in the text's rows"
                    want_of[turn % 3] = _in_layout(annotated, layout)
                s = _sink(n, h, w, layout, extra, offset)
                try:
                    b.upload_frames(frames, first=first)
                    b.overlay_run_to_surfaces(ps, s.frames, first=first, lines=ts, **TEXT_KW)
                    b.store_wait()
                    assert b.last_overlay_launches() == 1
                    s.check(want_of[turn % 3], (layout, size, n, extra, offset))
                finally:
                    s.close()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_another_matrix_and_no_text(layout):
    w, h = SIZE
    a, b = _small_ctx(SIZE, "rgb", 4), _small_ctx(SIZE, "rgb", 4)
    try:
        frames = _noise(3, h, w, "rgb", seed=5)
        ps, ts = _pick(0, 3, _polygons(w, h))
        annotated = _annotated(a, frames, ps, ts, first=1)
        s, t = _sink(3, h, w, layout, 16, 0), _sink(3, h, w, layout, 5, 1)
        try:
            b.upload_frames(frames, first=1)
            b.overlay_run_to_surfaces(ps, s.frames, first=1, lines=ts, matrix="bt709", **TEXT_KW)
            b.sync()                                                        # (lt_sync covers the draw as well)
            s.check(_in_layout(annotated, layout, "bt709"), "bt709")
            a.overlay_run(ps, first=1)                                      # the lane alone
            lane_only = a.download_overlay(3, first=1).copy()
            assert (lane_only != annotated).any()
            b.overlay_run_to_surfaces(ps, t.frames, first=1)
            b.store_wait()
            t.check(_in_layout(lane_only, layout), "no text")
        finally:
            s.close()
            t.close()
    finally:
        a.close()
        b.close()


# ---- 2. several calibration sets in one launch ---------------------------------------------------------------------------------------------
def _ctx_of_sets(minvs, capacity):
    c = _native.Context(SIZE, SIZE, np.eye(3), np.zeros(5), np.eye(3), capacity=capacity)
    try:
        for i in range(1, len(minvs)):
            assert c.add_calibration(np.eye(3), np.zeros(5), np.eye(3)) == i
        c.overlay_configure(minvs[0])                                       # set 0: lt_overlay_configure
        for i in range(1, len(minvs)):
            c.overlay_configure(minvs[i], calibration=i)                    # the others: lt_overlay_configure_set
        c.overlay_set_font(*FONT)
    except BaseException:
        c.close()
        raise
    return c


@pytest.fixture(scope="module")
def contexts():
    """One context with the three sets and three one-set contexts, 66 slots each."""
    made = []
    try:
        made.append(_ctx_of_sets(MINV, 66))
        for m in MINV:
            made.append(_ctx_of_sets([m], 66))
        yield made[0], made[1:]
    finally:
        for c in made:
            c.close()


def _cycle(items, n, shift=0):
    return [items[(i + shift) % len(items)] for i in range(n)]


class _SetBySet:
    """The slots of a mixed range as the one-set contexts compute them: every context over the whole range, slot j from set ids[j]."""

    def __init__(self, solos, frames, ps, ts, first):
        self.solos, self.frames, self.ps, self.ts, self.first = solos, frames, ps, ts, first
        self._with_text, self._lane = {}, {}

    def with_text(self, ids):
        for s in set(ids):
            if s not in self._with_text:
                self._with_text[s] = _annotated(self.solos[s], self.frames, self.ps, self.ts, first=self.first)
        return np.stack([self._with_text[s][j] for j, s in enumerate(ids)])

    def lane_only(self, ids):
        for s in set(ids):
            if s not in self._lane:
                self.solos[s].upload_frames(self.frames, first=self.first)
                self.solos[s].overlay_run(self.ps, first=self.first)
                self._lane[s] = self.solos[s].download_overlay(len(self.frames), first=self.first).copy()
        return np.stack([self._lane[s][j] for j, s in enumerate(ids)])


def test_a_range_of_several_sets_is_one_launch(contexts):
    mixed, solos = contexts
    w, h = SIZE
    first, ids = 1, [0, 1, 1, 2, 0]
    n = len(ids)
    frames = _noise(n, h, w, "rgb", seed=21)
    polys = _polygons(w, h)
    ps, ts = _cycle(polys, n), _cycle(TEXTS, n, 1)
    ref = _SetBySet(solos, frames, ps, ts, first)
    # a condition of the test: the sets draw different frames
    every = [ref.lane_only([s] * n) for s in range(3)]
    assert (every[0] != every[1]).any() and (every[0] != every[2]).any() and (every[1] != every[2]).any()
    want_text, want_lane = ref.with_text(ids), ref.lane_only(ids)
    try:
        mixed.upload_frames(frames, first=first)
        mixed.set_slot_calibrations(ids, first=first)
        # the fused draw into sinks
        for layout, extra, offset in (("rgb", 0, 0), ("nv12", 3, 1), ("i420", 0, 0)):
            s = _sink(n, h, w, layout, extra, offset)
            try:
                mixed.overlay_run_to_surfaces(ps, s.frames, first=first, lines=ts, **TEXT_KW)
                mixed.store_wait()
                assert mixed.last_overlay_launches() == 1
                s.check(_in_layout(want_text, layout), ("to surfaces", layout))
            finally:
                s.close()
        # whole annotated frames
        mixed.overlay_run(ps, first=first)
        assert mixed.last_overlay_launches() == 1
        assert np.array_equal(mixed.download_overlay(n, first=first), want_lane)
        # row runs: the rows asked for equal the whole frames' rows
        rows4 = np.array([3, 19, 22, 41], np.int32)
        mixed.overlay_run(ps, first=first, rows=rows4.ctypes.data)
        assert mixed.last_overlay_launches() == 1
        got = _native.pinned_empty((n, h, w, 3))
        got[...] = 0
        mixed.download_overlay_async(got, first=first, rows=rows4.ctypes.data)
        mixed.sync()
        mixed.download_overlay_wait()
        for r0, r1 in ((3, 19), (22, 41)):
            assert np.array_equal(got[:, r0:r1], want_lane[:, r0:r1]), (r0, r1)
        # in place, into attached RGB surfaces
        s = _Surfaces(frames, "rgb", 5, 1)
        try:
            mixed.attach_device_frames(s.frames, first=first)
            mixed.overlay_run_inplace(ps, first=first, lines=ts, **TEXT_KW)
            mixed.store_wait()
            assert mixed.last_overlay_launches() == 1
            s.check(want_text, "in place")
        finally:
            s.close()
        # a range of one set -- not set 0 -- is one launch of that set's tables
        mixed.upload_frames(frames, first=first)
        mixed.set_slot_calibrations([2] * n, first=first)
        mixed.overlay_run(ps, first=first)
        assert mixed.last_overlay_launches() == 1
        assert np.array_equal(mixed.download_overlay(n, first=first), ref.lane_only([2] * n))
        s = _sink(n, h, w, "rgb")
        try:
            mixed.overlay_run_to_surfaces(ps, s.frames, first=first, lines=ts, **TEXT_KW)
            mixed.store_wait()
            assert mixed.last_overlay_launches() == 1
            s.check(ref.with_text([2] * n), "one set")
        finally:
            s.close()
    finally:
        mixed.sync()
        mixed.set_slot_calibrations([0] * n, first=first)


def test_long_ranges_split_into_launches(contexts):
    mixed, solos = contexts
    w, h = SIZE
    polys = _polygons(w, h)
    frames = _noise(66, h, w, "rgb", seed=33)
    ps, ts = _cycle(polys, 66), _cycle(TEXTS, 66, 2)
    ids = _cycle([1, 2], 66)
    ref = _SetBySet(solos, frames, ps, ts, 0)
    want = ref.with_text(ids)
    try:
        # 34 slots into an RGB sink: 32 surfaces travel with a launch
        mixed.upload_frames(frames[:34])
        mixed.set_slot_calibrations(ids, first=0)
        s = _sink(34, h, w, "rgb", 16, 0)
        try:
            mixed.overlay_run_to_surfaces(ps[:34], s.frames, lines=ts[:34], **TEXT_KW)
            mixed.store_wait()
            assert mixed.last_overlay_launches() == 2
            s.check(want[:34], "34 slots")
        finally:
            s.close()
        # 66 attached slots in place: 64 set ids travel with a launch
        s = _Surfaces(frames, "rgb", 0, 0)
        try:
            mixed.attach_device_frames(s.frames)
            mixed.overlay_run_inplace(ps, lines=ts, **TEXT_KW)
            mixed.store_wait()
            assert mixed.last_overlay_launches() == 2
            s.check(want, "66 slots")
        finally:
            s.close()
    finally:
        mixed.sync()
        mixed.set_slot_calibrations([0] * 66, first=0)


# ---- 3. refusals, before any launch ------------------------------------------------------------------------------------------------------
def _raw_call(ctx, n, surfaces, layout, coeffs, first=0):
    """lt_overlay_run_to_surfaces with empty polygons and no text, as the ABI takes it -> its status."""
    zero = np.zeros(n, np.int32)
    k = None if coeffs is None else np.ascontiguousarray(coeffs, np.int32)
    return ctx.lib.lt_overlay_run_to_surfaces(ctx._h, first, n, zero.ctypes.data, zero.ctypes.data, None, None, 0.3, None,
                                              None if surfaces is None else surfaces.ctypes.data, layout, None if k is None else k.ctypes.data)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refusals_leave_everything_as_it_was(layout):
    w, h = SIZE
    a, b = _small_ctx(SIZE, "rgb", 4), _small_ctx(SIZE, "rgb", 4)
    odd = _small_ctx((63, 47), "rgb", 2)
    two = _native.Context(SIZE, SIZE, np.eye(3), np.zeros(5), np.eye(3), capacity=4)
    polys = _polygons(w, h)
    frames = _noise(2, h, w, "rgb", seed=9)
    ps, ts = [polys[0], polys[2]], TEXTS[:2]
    s, cam = _sink(2, h, w, layout, 3, 1), _Surfaces(frames, "rgb", 0, 0)
    bt601 = _native.rgb2yuv_coeffs("bt601")
    lid = _native.sink_format_id(layout)
    try:
        want = _in_layout(_annotated(a, frames, ps, ts), layout)
        b.upload_frames(frames)
        surf = np.ascontiguousarray(s.frames.surfaces)
        err = lambda: b.lib.lt_last_error().decode()
        assert _raw_call(b, 2, None, lid, bt601) == -1 and "null" in err()                       # null surfaces
        if layout != "rgb":
            odd.upload_frames(_noise(1, 47, 63, "rgb", seed=1))
            assert _raw_call(odd, 1, surf, lid, bt601) == -1 and "even" in err()                 # an odd size for 4:2:0
            assert odd.last_overlay_launches() == -1
            assert _raw_call(b, 2, surf, lid, None) == -1 and "coefficients" in err()            # no coefficients
            _refused("invalid", lambda: b.overlay_run_to_surfaces(ps, s.frames, matrix=[1 << 23] + [0] * 7))   # ... out of bounds
        low = surf.copy()
        low["pitch"] = (3 * w if layout == "rgb" else w) - 1
        assert _raw_call(b, 2, low, lid, bt601) == -1 and "pitch" in err()                       # a pitch below the row
        same = surf.copy()
        same[1] = same[0]
        assert _raw_call(b, 2, same, lid, bt601) == -1 and "overlaps" in err()                   # destinations that overlap
        for bad in (3, 4):                                                                       # packed 4:2:2 is no destination
            assert _raw_call(b, 2, surf, bad, bt601) == -1 and "input format only" in err()
        with pytest.raises(ValueError):
            b.overlay_run_to_surfaces(ps, DeviceFrames(surf, SIZE, "yuy2", owner=s.buf))
        b.attach_device_frames(cam.frames, first=2)                                              # an attached camera surface as the sink
        if layout == "rgb":
            _refused("invalid", lambda: b.overlay_run_to_surfaces(ps, cam.frames, lines=ts, **TEXT_KW))
        else:                                                                                    # (4:2:0 surfaces laid into its memory)
            inside = surf.copy()
            inside["pitch"], inside["chroma_pitch"] = w, (w if layout == "nv12" else w // 2)
            for k in range(2):
                inside["plane"][k] = [cam.buf.ptr + k * 2 * w * h + off for off in (0, w * h, w * h + w * h // 4)]
            assert _raw_call(b, 2, inside, lid, bt601) == -1
        assert "attached to slot 2" in err()
        _refused("invalid", lambda: b.overlay_run_to_surfaces(ps, s.frames, lines=ts, origin=(5, 3), step=6, line_len=8))   # lines that overlap
        _refused("invalid", lambda: b.overlay_run_to_surfaces(ps, s.frames[0:1]))                # one surface for two slots
        b.upload_frame_rows(frames[:1], first=1)                                                 # slot 1 holds part of its frame only
        _refused("state", lambda: b.overlay_run_to_surfaces(ps, s.frames, lines=ts, **TEXT_KW))
        b.upload_frames(frames)
        # a slot whose calibration set has no overlay table
        assert two.add_calibration(np.eye(3), np.zeros(5), np.eye(3)) == 1
        two.overlay_configure(np.eye(3))
        two.upload_frames(frames)
        two.set_slot_calibrations([0, 1])
        _refused("state", lambda: two.overlay_run_to_surfaces(ps, s.frames))
        assert two.last_overlay_launches() == -1
        b.sync()
        assert s.unchanged() and cam.unchanged()                                                 # nothing reached the surfaces
        assert b.last_overlay_launches() == -1                                                   # ... and nothing was launched
        b.overlay_run_to_surfaces(ps, s.frames, lines=ts, **TEXT_KW)                             # the context works
        b.store_wait()
        assert b.last_overlay_launches() == 1
        s.check(want, "after the refusals")
        assert _raw_call(b, 2, same, lid, bt601) == -1                                           # a refusal does not move the counter
        assert b.last_overlay_launches() == 1
        assert b.lib.lt_last_overlay_launches(None) == -2 ** 31                                  # LT_NO_CONTEXT
    finally:
        for c in (a, b, odd, two):
            c.close()
        s.close()
        cam.close()
