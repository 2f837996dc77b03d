"""The instruction budget of the raw Bayer walks with a colour stage -- k_raw_walk_rows<PATTERN, SRC, PER_SLOT, STAGES> with STAGES 2, over the
8-bit table form (STAGES 0), and STAGES 3, over the 10- / 12-bit one (STAGES 1) (k_frontend.hip), DESIGN.md section 4 -- on the generated gfx950 code
(hipcc cross-compiles; no GPU needed), from the one compile of k_frontend.hip that test_isa_guards.py makes and through the same tool,
tools/isa_split.py.

Per walk: the 12 vector-memory instructions of the table form it wraps -- the one load of the staging brings the curve along with the
table --; no scratch; no v_mul_lo_u32 (every product of the matrix is a 24-bit one with the coefficient a scalar operand); one barrier,
ahead of the walk's early return; per frame 16 one-byte LDS reads for the table and 12 for the curve (3 channels x 4 taps); and the VALU
instructions inside the per-frame loop as the compiler gives them on the finished code (ROCm 7.2), no margin: the wrapped forms' 190 / 177
plus 72 (six per channel and tap: two v_mul_i32_i24_sdwa, v_mad_i32_i24, v_add3_u32, v_ashrrev_i32, v_med3_i32) and 210 / 197 plus 84 (the
same, and one v_add_u32 per curve lookup: the base of the dynamic LDS)."""
import re

import pytest

import test_isa_guards as G
import test_raw_lut_isa as R

pytestmark = G.needs_hipcc

assert R.STAGES_LOOP_VALU[2] == {0: 262, 1: 249} and R.STAGES_LOOP_VALU[3] == {0: 294, 1: 281}      # SRC 0: surfaces, 1: the slots' staging frames
WRAPPED = {2: 0, 3: 1}                   # STAGES of a colour walk -> STAGES of the table form it wraps
BUDGET = R.walk_budget([2, 3])


def _wrapped_name(name):
    return name[:name.rindex(" ") + 1] + "%d>" % WRAPPED[R.stages_of(name)]


def _front():
    split, isa = G._isa_split(), G._isa(G.os.path.join(G.CSRC, "k_frontend.hip"))
    return split, split.table(isa), {split.kernel_name(n): k["insts"] for n, k in split.kernels(isa).items()}


def test_the_colour_walks_are_these_and_the_others_are_what_they_were():
    split, table, insts = _front()
    assert len(BUDGET) == 32
    assert sorted(n for n in table if "k_raw_walk_rows" in n and R.stages_of(n) in (2, 3)) == sorted(BUDGET)
    rows = sorted(n for n in insts if n.startswith("k_raw_rows_rgb<") and R.stages_of(n) in (2, 3))
    assert rows == R.row_names([2, 3]) and len(rows) == 32
    # nothing else under the two names, 16 of each per stage, and none of them counted among the walks that the other budget tests select
    R.assert_raw_kernels_are_these(table, insts)


def test_colour_walks_keep_their_budget():
    split, table, insts = _front()
    for name, cap in BUDGET.items():
        st = table[name]
        wrapped = table[_wrapped_name(name)]
        print(name, st)
        assert st["vmem"] == wrapped["vmem"] == 12, "%s: %d vector-memory instructions, budget 12" % (name, st["vmem"])
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["mul_lo"] == 0, "%s: %d v_mul_lo_u32" % (name, st["mul_lo"])
        assert st["loop_valu"] is not None, "%s: no per-frame loop found" % name
        assert st["loop_valu"] <= cap, "%s: %d VALU instructions per frame, budget %d" % (name, st["loop_valu"], cap)
        # one barrier, ahead of the first s_endpgm: table and curve are staged before any thread leaves
        assert sum(i.startswith("s_barrier") for i in insts[name]) == 1, name
        first_end = next(k for k, i in enumerate(insts[name]) if i.startswith("s_endpgm"))
        barrier = next(k for k, i in enumerate(insts[name]) if i.startswith("s_barrier"))
        assert barrier < first_end, name
        # the lookups of a frame: 16 in the table, 12 in the curve -- from LDS, not through the memory pipe
        loop = split.store_loop(insts[name])
        assert sum(i.startswith("ds_read_u8") for i in loop) == 28, (name, [i for i in loop if i.startswith("ds_")])
        assert not any(re.match(r"^(global|flat)_load", i) for i in loop), name
        # the matrix: 36 products a frame, each a 24-bit multiply or multiply-add; the clamp a median of three per channel and tap
        # (the wrapped form's own 24-bit multiplies, the windows' addresses, come on top)
        mul24 = lambda body: sum(bool(re.match(r"^v_(mul|mad)_i32_i24", i)) for i in body)
        assert mul24(loop) == mul24(split.store_loop(insts[_wrapped_name(name)])) + 36, name
        assert sum(i.startswith("v_med3_i32") for i in loop) == 12, name
