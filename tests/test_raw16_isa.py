"""The instruction budget of the 10- / 12-bit raw Bayer walks -- k_raw_walk_rows<PATTERN, SRC, PER_SLOT, STAGES> with STAGES 1, the wide
table alone (k_frontend.hip), DESIGN.md section 4 -- on the generated gfx950 code (hipcc cross-compiles; no GPU needed), from the one compile of k_frontend.hip that
test_isa_guards.py makes and through the same tool, tools/isa_split.py.

Per walk: 12 vector-memory instructions -- two remap-table reads, four 96-bit windows of one frame before the loop and four of the next
inside it, the store, and the one 16-byte load of the staging loop that brings the table to LDS (4 KB or 16 KB: `bits` is a run-time
argument, the loop runs once or four times); no scratch; no v_mul_lo_u32; the frames read in whole aligned dwords only, three at a time;
16 one-byte LDS reads per frame, the lookups; one barrier, ahead of the walk's early return; and the VALU instructions inside the
per-frame loop as the compiler gives them on the finished code (ROCm 7.2), no margin: the 8-bit table's 190 / 177 plus 20 (the second
v_alignbyte_b32 of each of the four windows, and sixteen v_and_b32: the mask of every site, where an 8-bit site is cut out by the SDWA
operand of its address add)."""
import re

import pytest

import test_isa_guards as G
import test_raw_lut_isa as R

pytestmark = G.needs_hipcc

assert R.STAGES_LOOP_VALU[1] == {0: 210, 1: 197}             # SRC 0: surfaces, 1: the slots' dword-aligned staging frames
BUDGET = R.walk_budget([1])


def _wide_walks():
    split, isa = G._isa_split(), G._isa(G.os.path.join(G.CSRC, "k_frontend.hip"))
    table = split.table(isa, "k_raw_walk_rows")
    return split, {n: st for n, st in table.items() if R.stages_of(n) == 1}, {split.kernel_name(n): k["insts"] for n, k in split.kernels(isa).items()}


def test_there_are_sixteen_wide_walks_beside_the_others():
    split, table, insts = _wide_walks()
    assert len(BUDGET) == 16 and sorted(table) == sorted(BUDGET), sorted(table)
    R.assert_raw_kernels_are_these(split.table(G._isa(G.os.path.join(G.CSRC, "k_frontend.hip"))), insts)   # 16 of each stage, the 50 plain walks
    rows = sorted(n for n in insts if n.startswith("k_raw_rows_rgb<") and R.stages_of(n) == 1)
    assert rows == R.row_names([1]) and len(rows) == 16


def test_wide_walks_keep_their_budget():
    split, table, insts = _wide_walks()
    for name, cap in BUDGET.items():
        st = table[name]
        print(name, st)
        assert st["vmem"] == 12, "%s: %d vector-memory instructions, budget 12" % (name, st["vmem"])
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["mul_lo"] == 0, "%s: %d v_mul_lo_u32" % (name, st["mul_lo"])
        assert st["loop_valu"] is not None, "%s: no per-frame loop found" % name
        assert st["loop_valu"] <= cap, "%s: %d VALU instructions per frame, budget %d" % (name, st["loop_valu"], cap)
        # the frames: whole aligned dwords, three per window, no byte or short loads (the 16-bit loads are the remap-table reads)
        loads = [i for i in insts[name] if re.match(r"^(buffer|global|flat)_load", i)]
        assert not any("ubyte" in i or "sbyte" in i for i in loads), (name, loads)
        assert sum("buffer_load_dwordx3" in i for i in loads) == 8, (name, loads)
        assert all("dwordx3" in i for i in loads if i.startswith("buffer_load")), (name, loads)
        assert sum("short" in i for i in loads) <= 2, (name, loads)
        assert sum(bool(re.match(r"^(global|flat)_load_dwordx4 ", i)) for i in loads) == 1, (name, loads)     # the table, 16 bytes at a time
        # the table: 16-byte pieces into LDS, one barrier, and 16 byte lookups per frame -- from LDS, not through the memory pipe
        assert sum(i.startswith("ds_write_b128") for i in insts[name]) == 1 and sum(i.startswith("s_barrier") for i in insts[name]) == 1, name
        loop = split.store_loop(insts[name])
        assert sum(i.startswith("ds_read_u8") for i in loop) == 16, (name, [i for i in loop if i.startswith("ds_")])
        assert not any(re.match(r"^(global|flat)_load", i) for i in loop), name
        # ... staged before the walk's early return: the barrier comes before the first s_endpgm
        first_end = next(k for k, i in enumerate(insts[name]) if i.startswith("s_endpgm"))
        barrier = next(k for k, i in enumerate(insts[name]) if i.startswith("s_barrier"))
        assert barrier < first_end, name
