"""What a raw Bayer context is conditioned with -- raw table, colour stage, shading map -- does not depend on how it got there: one
long-lived context per format walks a fixed sequence of setter calls, and after EVERY step (a) its getters return exactly what the
sequence says is set and (b) its front end (undistorted rows, R plane, Lab-b plane of four slots) equals, byte for byte, that of a context
without a history -- created fresh and brought to the same state by at most three setter calls in the order table, stage, map.

The walk (WALK, below) is written out.  Its steps cross each of the 24 directed edges of the on / off cube of (table, stage, map), replace
each part by another one while both other parts are set, and repeat a few settings that change nothing; tests/test_raw_setup_cpu.py
checks that coverage without a GPU.  Size A (64 x 48); frames, tables, stages and maps are those of the per-stage suites."""
import numpy as np
import pytest

import front_matrix as FM
import test_gpu_bayer_wide as BW
import test_gpu_raw_color as GC
import test_gpu_raw_packed as RP
import test_gpu_raw_shading as GS
from lane_tracker_amd import _native, utils

pytestmark = pytest.mark.gpu

N, FIRST = 4, 1
# A step names the part it sets -- T table, S colour stage, M shading map -- and to what: 1 or 2, two unlike values of the part, or 0: no table
# (8 bits) / back to the default table (10 / 12 bits), stage off, map off.  The state behind every step is in the comment: (T, S, M).
WALK = (
    "S1",    # 0 1 0
    "M1",    # 0 1 1
    "S0",    # 0 0 1
    "T0",    # 0 0 1   no table where there is none, under a map: the map's identity table stays staged
    "T1",    # 1 0 1
    "M0",    # 1 0 0
    "S2",    # 1 2 0
    "M2",    # 1 2 2
    "T2",    # 2 2 2   another table, stage and map set
    "S1",    # 2 1 2   another stage, table and map set
    "M1",    # 2 1 1   another map, table and stage set
    "M1",    # 2 1 1   the same map again
    "S0",    # 2 0 1
    "T0",    # 0 0 1
    "S1",    # 0 1 1
    "M0",    # 0 1 0
    "S0",    # 0 0 0
    "S0",    # 0 0 0   no stage where there is none
    "M1",    # 0 0 1
    "M2",    # 0 0 2   another map, alone
    "M0",    # 0 0 0
    "T2",    # 2 0 0
    "T1",    # 1 0 0   another table, alone
    "M2",    # 1 0 2
    "S2",    # 1 2 2
    "T0",    # 0 2 2
    "S1",    # 0 1 2   another stage, no table
    "T1",    # 1 1 2
    "T2",    # 2 1 2   another table, back
    "M1",    # 2 1 1
    "S2",    # 2 2 1
    "M0",    # 2 2 0
    "T0",    # 0 2 0
    "T2",    # 2 2 0
    "T2",    # 2 2 0   the same table again
    "S0",    # 2 0 0
    "M0",    # 2 0 0   no map where there is none
    "T0",    # 0 0 0
)


def states(walk=WALK):
    """-> the state (T, S, M) behind every step."""
    out, s = [], [0, 0, 0]
    for step in walk:
        s["TSM".index(step[0])] = int(step[1])
        out.append(tuple(s))
    return out


def _values(fmt, bits):
    """-> {part: (None, value 1, value 2)}."""
    tables = (GC.table8(), np.ascontiguousarray(GC.table8()[::-1, ::-1])) if bits == 8 else (BW.tables(bits)[0][1], BW.tables(bits)[2][1])
    return {"T": (None,) + tables, "S": (None, GC.stages()[2][1:], GC.stages()[3][1:]), "M": (None, GS.maps(bits)[2][1], GS.maps(bits)[3][1])}


def _set(ctx, part, value):
    if part == "T":
        ctx.set_raw_lut(value)
    elif part == "S":
        ctx.set_raw_color(*(value if value is not None else (None, None)), enable=value is not None)
    else:
        ctx.set_raw_shading(value)


def _check_getters(ctx, vals, bits, state, where):
    t, s, m = (vals[p][k] for p, k in zip("TSM", state))
    got_t, got_s, got_m = ctx.raw_lut(), ctx.get_raw_color(), ctx.get_raw_shading()
    if bits == 8 and t is None:
        assert got_t is None, "%s: a table is reported where none is set" % where
    else:
        assert got_t is not None and np.array_equal(got_t, utils.raw_lut(bits=bits) if t is None else t), "%s: the table reported" % where
    if s is None:
        assert got_s is None, "%s: a stage is reported where none is set" % where
    else:
        assert got_s is not None and np.array_equal(got_s[0], s[0]) and np.array_equal(got_s[1], s[1]), "%s: the stage reported" % where
    if m is None:
        assert got_m is None, "%s: a map is reported where none is set" % where
    else:
        assert got_m is not None and np.array_equal(got_m.mesh, m.mesh) and np.array_equal(got_m.black, m.black), "%s: the map reported" % where


def _walk(fmt, bits, make, front, frames):
    live = lambda: _native.device_cache_stats()["live_bytes"]
    base = live()
    vals, ids = _values(fmt, bits), FM.ids_pattern(N)
    refs = {}

    def reference(state):
        """The front end of a context without a history in `state`: made once, kept, never changed."""
        if state not in refs:
            c = make()
            try:
                for part, k in zip("TSM", state):
                    if k:
                        _set(c, part, vals[part][k])
                refs[state] = front(c, frames, ids)
            finally:
                c.close()
            for a in refs[state]:
                a.setflags(write=False)
        return refs[state]

    ctx = make()
    try:
        _check_getters(ctx, vals, bits, (0, 0, 0), "%s, a new context" % fmt)
        for k, (step, state) in enumerate(zip(WALK, states())):
            where = "%s, step %d (%s) -> table %d, stage %d, map %d" % ((fmt, k, step) + state)
            _set(ctx, step[0], vals[step[0]][int(step[1])])
            _check_getters(ctx, vals, bits, state, where)
            got, want = front(ctx, frames, ids), reference(state)
            for what, g, p in zip(("undistorted rows", "R plane", "Lab-b plane"), got, want):
                assert g.shape == p.shape and np.array_equal(g, p), "%s: %d bytes of the %s differ from those of a context set up afresh" % (
                    where, int((g != p).sum()), what)
        # the states are not all one picture: the comparison above can tell them apart
        assert len({refs[s][0].tobytes() for s in refs}) == len(refs) == len(set(states()))
    finally:
        ctx.close()
    assert live() == base, fmt


def test_an_8_bit_context_is_what_its_setters_last_said():
    fmt = "bayer_grbg"
    _walk(fmt, 8, lambda: BW._context(fmt, "A"), lambda c, f, ids: BW._front(c, fmt, f, ids, FIRST, "upload"), FM.frame_pool(fmt, "A")[:N])


def test_a_12_bit_context_is_what_its_setters_last_said():
    fmt = "bayer12_grbg"
    _walk(fmt, 12, lambda: BW._context(fmt, "A"), lambda c, f, ids: BW._front(c, fmt, f, ids, FIRST, "upload"), BW.wide_pool("bayer_grbg", 12, "A")[3:3 + N])


def test_a_packed_10_bit_context_is_what_its_setters_last_said():
    fmt, wh = RP.names("bayer_grbg", 10)[0], FM.SIZES["A"]
    frames = utils.pack_raw(RP.pool(10, wh)[4:4 + N], fmt)
    _walk(fmt, 10, lambda: RP._context(fmt, wh), lambda c, f, ids: RP._front(c, fmt, f, ids, FIRST, "upload"), frames)
