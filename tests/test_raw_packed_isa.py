"""The instruction budget of the walks over MIPI-packed RAW10 / RAW12 frames -- k_mipi_walk_rows<PATTERN, SRC, PER_SLOT, STAGES, PACK>
(k_frontend.hip; STAGES 1, 3, 5, 7 as k_raw_walk_rows has them: the wide table, + colour stage, + shading map, + both; PACK 0: RAW10, 1:
RAW12), DESIGN.md section 4 -- on the generated gfx950 code (hipcc cross-compiles; no GPU needed), from the one compile of k_frontend.hip
that test_isa_guards.py makes and through the same tool, tools/isa_split.py.

Per walk, against the 16-bit form it unpacks into (k_raw_walk_rows<.., STAGES>): that form's vector-memory instructions -- 12, with the
shading map 16 --, the frames in eight aligned 96-bit loads (buffer_load_dwordx3; the gain window's four are the same instruction: 12 with a
map) and in no byte or short load; no scratch; no v_mul_lo_u32; the 16-bit form's LDS accesses per frame, the 16 one-byte table lookups
(and the colour stage's 12 of the curve); one barrier, ahead of the walk's early return; nothing but the windows from memory inside the
per-frame loop.  What a frame adds is VALU work alone: per window row the third v_alignbyte_b32 (RAW10), four v_perm_b32 and two
v_pk_lshrrev_b16 with selectors and shifts found once per walk, the masks and shift-ors -- and RAW10's one select of the dword that holds the
low bits of the window's last site.  The VALU instructions inside the per-frame loop and the VGPRs are pinned at what the compiler gives on
the finished code (ROCm 7.2), no margin (SRC surfaces / slots):

    STAGES            RAW10: loop VALU   VGPRs      RAW12: loop VALU   VGPRs      16-bit words: loop VALU   VGPRs
    1  table            266 / 253       69 / 67       258 / 245       68 / 66          210 / 197          54 / 53
    3  + colour         350 / 337       69 / 68       342 / 329       69 / 67          294 / 281          55 / 54
    5  + shading        346 / 333       93 / 87       338 / 325       92 / 85          290 / 277          78 / 77
    7  + both           430 / 417       94 / 93       422 / 409       93 / 92          374 / 361          79 / 78

RAW10 adds 56 a frame, 14 a window row; RAW12 48, 12 a row.  The packed forms hold a window row in three dwords where the 16-bit forms hold
two: 12 to 15 more VGPRs, and with the shading map the forms pass 80, where a SIMD holds one wave fewer than for the 16-bit forms."""
import re

import pytest

import test_isa_guards as G
import test_raw_lut_isa as R

pytestmark = G.needs_hipcc

# (STAGES, PACK) -> {SRC: (loop VALU, VGPRs)}; SRC 0: surfaces, 1: the slots' staging frames
FORMS = {(1, 0): {0: (266, 69), 1: (253, 67)}, (1, 1): {0: (258, 68), 1: (245, 66)},
         (3, 0): {0: (350, 69), 1: (337, 68)}, (3, 1): {0: (342, 69), 1: (329, 67)},
         (5, 0): {0: (346, 93), 1: (333, 87)}, (5, 1): {0: (338, 92), 1: (325, 85)},
         (7, 0): {0: (430, 94), 1: (417, 93)}, (7, 1): {0: (422, 93), 1: (409, 92)}}
ADDS = {0: 56, 1: 48}                                              # VALU instructions a frame over the 16-bit form, by PACK


def walk_name(p, src, per_slot, stages, pack):
    return "k_mipi_walk_rows<%d, %d, %s, %d, %d>" % (p, src, per_slot, stages, pack)


# name of a packed walk -> (name of the 16-bit walk, loop VALU, VGPRs, STAGES, PACK)
BUDGET = {walk_name(p, src, per_slot, st, pack): (R.walk_name(p, src, per_slot, st), valu, vgpr, st, pack)
          for (st, pack), caps in FORMS.items() for p in range(4) for src, (valu, vgpr) in caps.items() for per_slot in ("false", "true")}
ROWS = sorted("k_mipi_rows_rgb<%d, %s, %s, %d, %d>" % (p, s, w, st, pack)
              for st in (1, 3, 5, 7) for pack in (0, 1) for p in range(4) for s in ("false", "true") for w in ("false", "true"))


def _front():
    split, isa = G._isa_split(), G._isa(G.os.path.join(G.CSRC, "k_frontend.hip"))
    return split, split.table(isa), {split.kernel_name(n): k["insts"] for n, k in split.kernels(isa).items()}


def test_the_packed_kernels_are_these_and_the_others_are_what_they_were():
    split, table, insts = _front()
    assert len(BUDGET) == 128 and len(ROWS) == 128
    assert sorted(n for n in table if "k_mipi_walk_rows" in n) == sorted(BUDGET)
    assert sorted(n for n in table if "k_mipi_rows_rgb" in n) == ROWS
    assert not [n for n in table if "mipi" in n and n not in BUDGET and n not in ROWS]
    # the pinned sets under the other names: 128 + 128 raw kernels, 50 plain walks; no new name is counted among them
    R.assert_raw_kernels_are_these(table, insts)
    for n in list(BUDGET) + ROWS:
        assert "k_raw_walk_rows" not in n and "k_raw_rows_rgb" not in n and "k_undistort_rows" not in n
        assert not re.match(r"k_(raw16|cc|cc16|ls|ls16)_", n)
    # the packed forms agree with the 16-bit forms' counts that this file is stated against
    for (st, pack), caps in FORMS.items():
        assert {src: valu - ADDS[pack] for src, (valu, _) in caps.items()} == R.STAGES_LOOP_VALU[st], (st, pack)
    # the row conversions: no scratch, no v_mul_lo_u32
    for n in ROWS:
        assert table[n]["scratch"] == 0 and table[n]["mul_lo"] == 0, (n, table[n])


def test_packed_walks_keep_their_budget():
    split, table, insts = _front()
    vmem = lambda body: sum(bool(re.match(r"^(buffer|global|flat|scratch)_", i)) for i in body)
    lds = lambda body: sum(i.startswith("ds_") for i in body)
    for name, (wide, valu, vgpr, stages, pack) in BUDGET.items():
        st, ws = table[name], table[wide]
        shaded, coloured = bool(stages & 4), bool(stages & 2)
        print(name, st)
        assert st["vmem"] == ws["vmem"] == (16 if shaded else 12), "%s: %d vector-memory instructions, the 16-bit walk has %d" % (name, st["vmem"], ws["vmem"])
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["mul_lo"] == 0, "%s: %d v_mul_lo_u32" % (name, st["mul_lo"])
        assert st["loop_valu"] is not None, "%s: no per-frame loop found" % name
        assert ws["loop_valu"] == R.STAGES_LOOP_VALU[stages][int(name.split(", ")[1])], "%s: the 16-bit form's count in this file is stale" % wide
        assert st["loop_valu"] == valu == ws["loop_valu"] + ADDS[pack], "%s: %d VALU instructions per frame, pinned at %d" % (name, st["loop_valu"], valu)
        assert st["vgpr"] == vgpr, "%s: %d VGPRs, pinned at %d" % (name, st["vgpr"], vgpr)
        # the frames: eight aligned 96-bit loads (four windows before the loop, four of the next frame inside it; the gain window's four
        # are the same instruction), no byte load, and the one 16-bit load that is a remap-table read
        loads = [i for i in insts[name] if re.match(r"^(buffer|global|flat)_load", i)]
        assert sum("buffer_load_dwordx3" in i for i in loads) == (12 if shaded else 8), (name, loads)
        assert not any("ubyte" in i or "sbyte" in i for i in loads), (name, loads)
        assert sum("short" in i for i in loads) == sum("short" in i for i in insts[wide] if re.match(r"^(buffer|global|flat)_load", i)) == 1, (name, loads)
        assert not any("buffer_load_dwordx2" in i or "buffer_load_dword " in i for i in loads), (name, loads)
        # one barrier, ahead of the first s_endpgm: the table is staged before any thread leaves
        assert sum(i.startswith("s_barrier") for i in insts[name]) == 1, name
        first_end = next(k for k, i in enumerate(insts[name]) if i.startswith("s_endpgm"))
        barrier = next(k for k, i in enumerate(insts[name]) if i.startswith("s_barrier"))
        assert barrier < first_end, name
        # the per-frame loop: the 16-bit form's memory instructions (four windows, the store) and LDS accesses -- 16 one-byte table
        # lookups, and the colour stage's 12 of the curve -- and nothing else that is not VALU or scalar
        loop, wloop = split.store_loop(insts[name]), split.store_loop(insts[wide])
        assert vmem(loop) == vmem(wloop) == 5, (name, vmem(loop), vmem(wloop))
        assert sum("buffer_load_dwordx3" in i for i in loop) == 4, name
        assert not any(re.match(r"^(global|flat)_load", i) for i in loop), name
        assert lds(loop) == lds(wloop) == sum(i.startswith("ds_read_u8") for i in loop) == (28 if coloured else 16), (name, lds(loop), lds(wloop))
        # what unpacks: per window row four byte permutes and two packed shifts, with per-walk selectors
        assert sum(i.startswith("v_perm_b32") for i in loop) == 16 and sum(i.startswith("v_pk_lshrrev_b16") for i in loop) == 8, name
        assert sum(i.startswith("v_alignbyte_b32") for i in loop) == (12 if pack == 0 else 8), name
