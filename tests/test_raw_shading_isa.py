"""The instruction budget of the raw Bayer walks behind the lens-shading correction -- k_raw_walk_rows<PATTERN, SRC, PER_SLOT, STAGES> with
STAGES 4 over the 8-bit table form and 5 over the 10- / 12-bit one, 6 and 7 the same with the colour stage (k_frontend.hip; the names
below are the ones these kernels had as families of their own: k_ls = 4, k_ls16 = 5, with CC 6 and 7, wrapping k_raw = 0, k_raw16 = 1,
k_cc = 2, k_cc16 = 3), DESIGN.md section 4 -- on the generated gfx950 code (hipcc cross-compiles; no GPU needed), from the one compile of
k_frontend.hip that test_isa_guards.py makes and through the same tool, tools/isa_split.py.

Per walk, against the form it wraps (k_raw_walk_rows / k_raw16_walk_rows; CC: k_cc_walk_rows / k_cc16_walk_rows): 16 vector-memory
instructions, the wrapped form's 12 plus the four loads of the gain window, which are outside the per-frame loop -- the loop has the
wrapped form's 5 --; no scratch; no v_mul_lo_u32; the wrapped form's one barrier, ahead of the walk's early return; in the loop 16 more
24-bit multiply-adds (one per site) and the wrapped form's LDS reads.  The VALU instructions inside the per-frame loop and the VGPRs are
pinned at what the compiler gives on the finished code (ROCm 7.2), no margin (SRC surfaces / slots):

    form                      loop VALU    VGPRs       wrapped: loop VALU   VGPRs
    k_ls_walk_rows              262 / 249   77 / 76     k_raw_walk_rows     190 / 177   50 / 49
    k_ls_walk_rows, CC          334 / 321   77 / 76     k_cc_walk_rows      262 / 249   51 / 50
    k_ls16_walk_rows            290 / 277   78 / 77     k_raw16_walk_rows   210 / 197   54 / 53
    k_ls16_walk_rows, CC        374 / 361   79 / 78     k_cc16_walk_rows    294 / 281   55 / 54

8 bits: + 72 a frame, 4.5 a site -- v_sub_u32 (the sample an SDWA byte select), v_mad_i32_i24, v_ashrrev_i32, v_med3_i32, and for 8 of
the 16 gains a v_and_b32 / v_lshrrev_b32 that takes the gain out of its dword.  10 / 12 bits: + 80, 5 a site -- v_sub_u32, v_mad_i32_i24,
v_ashrrev_i32 and, smax being a run-time value, v_max_i32 + v_min_i32 for the clamp; the gains' halves are operand selects.  The 24 to 27
more VGPRs are the 8 that hold the 16 gains, the 8 of the window's pedestals and their rounding terms (selected per thread by the window's
parities), and what the longer expression keeps live; no form passes 80, where a SIMD holds one wave fewer."""
import re

import pytest

import test_isa_guards as G
import test_raw_lut_isa as R

pytestmark = G.needs_hipcc

# STAGES of a shading walk -> (STAGES of the form it wraps, {SRC: (loop VALU, VGPRs)}); SRC 0: surfaces, 1: the slots' staging frames
FORMS = {4: (0, {0: (262, 77), 1: (249, 76)}),
         6: (2, {0: (334, 77), 1: (321, 76)}),
         5: (1, {0: (290, 78), 1: (277, 77)}),
         7: (3, {0: (374, 79), 1: (361, 78)})}
WRAPPED_VALU = {0: {0: 190, 1: 177}, 2: {0: 262, 1: 249}, 1: {0: 210, 1: 197}, 3: {0: 294, 1: 281}}
assert all(R.STAGES_LOOP_VALU[w] == v for w, v in WRAPPED_VALU.items())
assert all(R.STAGES_LOOP_VALU[st] == {src: valu for src, (valu, _) in caps.items()} for st, (_, caps) in FORMS.items())
# name of a walk -> (name of the wrapped walk, loop VALU, VGPRs, the wrapped walk's loop VALU)
BUDGET = {R.walk_name(p, src, per_slot, st): (R.walk_name(p, src, per_slot, w), valu, vgpr, WRAPPED_VALU[w][src])
          for st, (w, caps) in FORMS.items() for p in range(4) for src, (valu, vgpr) in caps.items() for per_slot in ("false", "true")}


def _front():
    split, isa = G._isa_split(), G._isa(G.os.path.join(G.CSRC, "k_frontend.hip"))
    return split, split.table(isa), {split.kernel_name(n): k["insts"] for n, k in split.kernels(isa).items()}


def test_the_shading_kernels_are_these_and_the_others_are_what_they_were():
    split, table, insts = _front()
    assert len(BUDGET) == 64
    assert sorted(n for n in table if "k_raw_walk_rows" in n and R.stages_of(n) >= 4) == sorted(BUDGET)
    rows = sorted(n for n in insts if n.startswith("k_raw_rows_rgb<") and R.stages_of(n) >= 4)
    assert rows == R.row_names([4, 5, 6, 7]) and len(rows) == 64
    assert sum(n.startswith("k_shade_expand") for n in insts) == 1
    # nothing else under the two names; the forms without a map are the 16 walks and 16 row kernels of each of STAGES 0 .. 3 (64 with a
    # colour stage or without); and no name of them is counted among the kernels that the other budget tests select
    R.assert_raw_kernels_are_these(table, insts)
    assert sum(R.stages_of(n) in (2, 3) for n in insts if "k_raw_walk_rows" in n or n.startswith("k_raw_rows_rgb<")) == 64
    # the row conversions: no scratch, no v_mul_lo_u32
    for n in rows:
        assert table[n]["scratch"] == 0 and table[n]["mul_lo"] == 0, (n, table[n])


def test_shading_walks_keep_their_budget():
    split, table, insts = _front()
    vmem = lambda body: sum(bool(re.match(r"^(buffer|global|flat|scratch)_", i)) for i in body)
    mul24 = lambda body: sum(bool(re.match(r"^v_(mul|mad)_i32_i24", i)) for i in body)
    lds = lambda body: sum(i.startswith("ds_") for i in body)
    for name, (wrapped, valu, vgpr, wrapped_valu) in BUDGET.items():
        st, ws = table[name], table[wrapped]
        print(name, st)
        assert st["vmem"] == ws["vmem"] + 4 == 16, "%s: %d vector-memory instructions, budget 16" % (name, st["vmem"])
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["mul_lo"] == 0, "%s: %d v_mul_lo_u32" % (name, st["mul_lo"])
        assert st["loop_valu"] is not None, "%s: no per-frame loop found" % name
        assert ws["loop_valu"] == wrapped_valu, "%s: the wrapped form's count in this file is stale" % wrapped
        assert st["loop_valu"] == valu, "%s: %d VALU instructions per frame, pinned at %d" % (name, st["loop_valu"], valu)
        assert st["vgpr"] == vgpr, "%s: %d VGPRs, pinned at %d" % (name, st["vgpr"], vgpr)
        # the wrapped form's barriers, in its place: ahead of the first s_endpgm -- the table is staged before any thread leaves
        assert sum(i.startswith("s_barrier") for i in insts[name]) == sum(i.startswith("s_barrier") for i in insts[wrapped]) == 1, name
        first_end = next(k for k, i in enumerate(insts[name]) if i.startswith("s_endpgm"))
        barrier = next(k for k, i in enumerate(insts[name]) if i.startswith("s_barrier"))
        assert barrier < first_end, name
        # the per-frame loop: the wrapped form's vector-memory instructions and LDS reads, nothing from global memory beside the windows;
        # the gains' four loads are in front of it
        loop, wloop = split.store_loop(insts[name]), split.store_loop(insts[wrapped])
        assert vmem(loop) == vmem(wloop) == 5, (name, vmem(loop), vmem(wloop))
        assert lds(loop) == lds(wloop), (name, lds(loop), lds(wloop))
        assert not any(re.match(r"^(global|flat)_load", i) for i in loop), name
        # one 24-bit multiply-add per site and frame
        assert mul24(loop) == mul24(wloop) + 16, (name, mul24(loop), mul24(wloop))
