"""The instruction budget of the conditioned raw Bayer walks -- k_raw_walk_rows<PATTERN, SRC, PER_SLOT, STAGES> with STAGES 0, the 8-bit
table alone (k_frontend.hip), DESIGN.md section 4 -- on the generated gfx950 code (hipcc cross-compiles; no GPU needed), from the one compile of k_frontend.hip that
test_isa_guards.py makes and through the same tool, tools/isa_split.py.

Per walk: 12 vector-memory instructions -- raw Bayer's 11 (two remap-table reads, four windows of one frame before the loop and four of
the next inside it, the store) and the one dword of the raw table that each of the workgroup's 256 threads brings to LDS; no scratch;
no v_mul_lo_u32; the frames read in whole aligned dwords only; 16 one-byte LDS reads per frame, the lookups; and the VALU instructions
inside the per-frame loop as the compiler gives them on the finished code (ROCm 7.2), no margin: plain raw Bayer's 158 / 145 plus 32.

This file also holds what the budget files of the other stages (test_raw16_isa, test_raw_color_isa, test_raw_shading_isa) share: the names of
the one raw walk and the one raw row kernel per STAGES value -- bit 0: 16-bit samples, bit 1: the colour stage, bit 2: the shading map -- and
the walks' VALU instructions per frame."""
import re

import pytest

import test_isa_guards as G

pytestmark = G.needs_hipcc

# STAGES -> {SRC: VALU instructions inside the per-frame loop}; SRC 0: surfaces, 1: the slots' dword-aligned staging frames
STAGES_LOOP_VALU = {0: {0: 190, 1: 177}, 1: {0: 210, 1: 197}, 2: {0: 262, 1: 249}, 3: {0: 294, 1: 281},
                    4: {0: 262, 1: 249}, 5: {0: 290, 1: 277}, 6: {0: 334, 1: 321}, 7: {0: 374, 1: 361}}


def walk_name(p, src, per_slot, stages):
    return "k_raw_walk_rows<%d, %d, %s, %d>" % (p, src, per_slot, stages)


def walk_budget(stages):
    """name of a walk -> its loop VALU, for the 16 walks of each of `stages`"""
    return {walk_name(p, src, per_slot, st): cap
            for st in stages for p in range(4) for src, cap in STAGES_LOOP_VALU[st].items() for per_slot in ("false", "true")}


def row_names(stages):
    return sorted("k_raw_rows_rgb<%d, %s, %s, %d>" % (p, s, w, st) for st in stages for p in range(4) for s in ("false", "true") for w in ("false", "true"))


def stages_of(name):
    return int(name[name.rindex(" ") + 1:-1])


def assert_raw_kernels_are_these(table, insts):
    """16 walks and 16 row kernels per STAGES value, 128 of each in all, nothing else under the two names; the 50 plain walks beside them."""
    walks = sorted(n for n in table if "k_raw_walk_rows" in n)
    rows = sorted(n for n in insts if "k_raw_rows_rgb" in n)
    assert walks == sorted(walk_budget(range(8))) and len(walks) == 128
    assert rows == row_names(range(8)) and len(rows) == 128
    for st in range(8):
        assert sum(stages_of(n) == st for n in walks) == 16 and sum(stages_of(n) == st for n in rows) == 16, st
    # the names the six-kernel families had are gone: everything raw is one of the two above
    assert not [n for n in insts if re.match(r"k_(raw16|cc|cc16|ls|ls16)_", n)]
    assert len(G._walks()[0]) == 50                               # (a name that held k_undistort_rows would have been counted there)


BUDGET = walk_budget([0])


def _raw_walks():
    split, isa = G._isa_split(), G._isa(G.os.path.join(G.CSRC, "k_frontend.hip"))
    return split, split.table(isa, "k_raw_walk_rows"), {split.kernel_name(n): k["insts"] for n, k in split.kernels(isa).items()}


def test_there_are_sixteen_conditioned_walks_and_fifty_plain_ones():
    _, table, insts = _raw_walks()
    assert len(BUDGET) == 16 and sorted(n for n in table if stages_of(n) == 0) == sorted(BUDGET), sorted(table)
    assert_raw_kernels_are_these(table, insts)


def test_conditioned_walks_keep_their_budget():
    split, table, insts = _raw_walks()
    for name, cap in BUDGET.items():
        st = table[name]
        print(name, st)
        assert st["vmem"] == 12, "%s: %d vector-memory instructions, budget 12" % (name, st["vmem"])
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["mul_lo"] == 0, "%s: %d v_mul_lo_u32" % (name, st["mul_lo"])
        assert st["loop_valu"] is not None, "%s: no per-frame loop found" % name
        assert st["loop_valu"] <= cap, "%s: %d VALU instructions per frame, budget %d" % (name, st["loop_valu"], cap)
        # the frames: whole aligned dwords, no byte or short loads (the one 16-bit load is a remap-table read)
        loads = [i for i in insts[name] if re.match(r"^(buffer|global|flat)_load", i)]
        assert not any("ubyte" in i or "sbyte" in i for i in loads), (name, loads)
        assert sum("buffer_load_dwordx2" in i for i in loads) == 8, (name, loads)
        assert sum(bool(re.match(r"^(global|flat)_load_dword ", i)) for i in loads) >= 1, (name, loads)     # the table's dword
        # the table: one dword a thread into LDS, one barrier, and 16 byte lookups per frame -- from LDS, not through the memory pipe
        assert sum(i.startswith("ds_write_b32") for i in insts[name]) == 1 and sum(i.startswith("s_barrier") for i in insts[name]) == 1, name
        loop = split.store_loop(insts[name])
        assert sum(i.startswith("ds_read_u8") for i in loop) == 16, (name, [i for i in loop if i.startswith("ds_")])
        # ... staged before the walk's early return: the barrier comes before the first s_endpgm
        first_end = next(k for k, i in enumerate(insts[name]) if i.startswith("s_endpgm"))
        barrier = next(k for k, i in enumerate(insts[name]) if i.startswith("s_barrier"))
        assert barrier < first_end, name
