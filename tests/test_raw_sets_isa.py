"""The instruction budget of the set-per-slot raw kernels -- k_rawset_walk_rows<PATTERN, SRC, STAGES>, k_packset_walk_rows<PATTERN, SRC, STAGES,
PACK> and the row conversions k_rawset_rows_rgb / k_packset_rows_rgb (k_frontend.hip), DESIGN.md section 4 -- on the generated gfx950 code
(hipcc cross-compiles; no GPU needed), from the one compile of k_frontend.hip that test_isa_guards.py makes and through the same tool,
tools/isa_split.py.

A set-per-slot walk is the one-set walk in its table-per-slot form (k_raw_walk_rows / k_mipi_walk_rows<.., true, ..>) of the same STAGES
behind a prologue that finds its slot's raw set: per walk and per frame it adds NO vector-memory instruction, no LDS instruction and no VALU
instruction inside the frame loop, no VGPR, no scratch, no v_mul_lo_u32 and no barrier; what it adds is scalar loads (the set's id is a
byte of the kernel argument, the entry 80 bytes of device memory).  The counts below are this build's (ROCm 7.2), no margin; those of the
byte and word walks are test_raw_lut_isa.STAGES_LOOP_VALU's, as they must be.

    STAGES   k_rawset_walk_rows: loop VALU, VGPRs (SRC surfaces / slots)      k_packset_walk_rows: RAW10 ...            RAW12 ...
    0        190 / 177   50 / 49
    1        210 / 197   54 / 53                                              266 / 253   69 / 67                       258 / 245   68 / 66
    2        262 / 249   51 / 50
    3        294 / 281   55 / 54                                              350 / 337   69 / 68                       342 / 329   69 / 67
    4        262 / 249   77 / 76
    5        290 / 277   78 / 77                                              346 / 333   93 / 87                       338 / 325   92 / 85
    6        334 / 321   77 / 76
    7        374 / 361   79 / 78                                              430 / 417   94 / 93                       422 / 409   93 / 92

This check looks at instruction classes and counts and at nothing else."""
import re

import test_isa_guards as G
import test_raw_lut_isa as R

pytestmark = G.needs_hipcc

# STAGES -> {SRC: (loop VALU, VGPRs)}
RAWSET = {0: {0: (190, 50), 1: (177, 49)}, 1: {0: (210, 54), 1: (197, 53)}, 2: {0: (262, 51), 1: (249, 50)}, 3: {0: (294, 55), 1: (281, 54)},
          4: {0: (262, 77), 1: (249, 76)}, 5: {0: (290, 78), 1: (277, 77)}, 6: {0: (334, 77), 1: (321, 76)}, 7: {0: (374, 79), 1: (361, 78)}}
# (STAGES, PACK) -> {SRC: (loop VALU, VGPRs)}
PACKSET = {(1, 0): {0: (266, 69), 1: (253, 67)}, (1, 1): {0: (258, 68), 1: (245, 66)}, (3, 0): {0: (350, 69), 1: (337, 68)},
           (3, 1): {0: (342, 69), 1: (329, 67)}, (5, 0): {0: (346, 93), 1: (333, 87)}, (5, 1): {0: (338, 92), 1: (325, 85)},
           (7, 0): {0: (430, 94), 1: (417, 93)}, (7, 1): {0: (422, 93), 1: (409, 92)}}
# name of a set-per-slot walk -> (name of the one-set walk in its table-per-slot form, loop VALU, VGPRs)
WALKS = {"k_rawset_walk_rows<%d, %d, %d>" % (p, src, st): (R.walk_name(p, src, "true", st), valu, vgpr)
         for st, caps in RAWSET.items() for p in range(4) for src, (valu, vgpr) in caps.items()}
WALKS.update({"k_packset_walk_rows<%d, %d, %d, %d>" % (p, src, st, pack): ("k_mipi_walk_rows<%d, %d, true, %d, %d>" % (p, src, st, pack), valu, vgpr)
              for (st, pack), caps in PACKSET.items() for p in range(4) for src, (valu, vgpr) in caps.items()})
ROWS = sorted(["k_rawset_rows_rgb<%d, %s, %s, %d>" % (p, s, w, st) for st in range(8) for p in range(4) for s in ("false", "true") for w in ("false", "true")] +
              ["k_packset_rows_rgb<%d, %s, %s, %d, %d>" % (p, s, w, st, pack) for st in (1, 3, 5, 7) for pack in (0, 1) for p in range(4)
               for s in ("false", "true") for w in ("false", "true")])
assert all(RAWSET[st] and {src: v for src, (v, _) in RAWSET[st].items()} == R.STAGES_LOOP_VALU[st] for st in range(8))


def _front():
    split, isa = G._isa_split(), G._isa(G.os.path.join(G.CSRC, "k_frontend.hip"))
    return split, split.table(isa), {split.kernel_name(n): k["insts"] for n, k in split.kernels(isa).items()}


def test_the_set_per_slot_kernels_are_these():
    _, table, insts = _front()
    assert len(WALKS) == 128 and len(ROWS) == 256
    assert sorted(n for n in table if "set_walk_rows" in n) == sorted(WALKS)
    assert sorted(n for n in insts if "set_rows_rgb" in n) == ROWS
    # none of them under a name the other budget files select by
    for n in list(WALKS) + ROWS:
        assert "k_raw_walk_rows" not in n and "k_raw_rows_rgb" not in n and "k_mipi" not in n and "k_undistort_rows" not in n
    for n in ROWS:
        assert table[n]["scratch"] == 0 and table[n]["mul_lo"] == 0, (n, table[n])


def test_a_set_per_slot_walk_is_its_one_set_walk_behind_a_scalar_prologue():
    split, table, insts = _front()
    vmem = lambda body: sum(bool(re.match(r"^(buffer|global|flat|scratch)_", i)) for i in body)
    lds = lambda body: sum(i.startswith("ds_") for i in body)
    valu = lambda body: sum(i.startswith("v_") for i in body)
    scalar_loads = lambda body: sum(bool(re.match(r"^s_(buffer_)?load_", i)) for i in body)
    barriers = lambda body: sum(i.startswith("s_barrier") for i in body)
    for name, (one, loop_valu, vgpr) in WALKS.items():
        st, os_ = table[name], table[one]
        print(name, st)
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["mul_lo"] == os_["mul_lo"] == 0, name
        assert st["vmem"] == os_["vmem"], "%s: %d vector-memory instructions, the one-set form has %d" % (name, st["vmem"], os_["vmem"])
        assert st["loop_valu"] == os_["loop_valu"] == loop_valu, "%s: %s VALU instructions per frame, the one-set form %s, recorded %d" % (
            name, st["loop_valu"], os_["loop_valu"], loop_valu)
        assert st["vgpr"] == os_["vgpr"] == vgpr, "%s: %d VGPRs, the one-set form %d, recorded %d" % (name, st["vgpr"], os_["vgpr"], vgpr)
        loop, oloop = split.store_loop(insts[name]), split.store_loop(insts[one])
        assert vmem(loop) == vmem(oloop) == 5, (name, vmem(loop), vmem(oloop))
        assert lds(loop) == lds(oloop) and lds(insts[name]) == lds(insts[one]), (name, lds(loop), lds(oloop))
        assert valu(loop) == valu(oloop), name
        assert scalar_loads(loop) == scalar_loads(oloop), name
        # the whole extra cost: scalar loads in front of the loop -- the id's dword and the entry
        extra = scalar_loads(insts[name]) - scalar_loads(insts[one])
        assert 1 <= extra <= 3, "%s: %d scalar loads more than the one-set form" % (name, extra)
        # the one barrier of the staging, ahead of the first exit: the table is staged before any thread leaves
        assert barriers(insts[name]) == barriers(insts[one]) == 1, name
        first_end = next(k for k, i in enumerate(insts[name]) if i.startswith("s_endpgm"))
        assert next(k for k, i in enumerate(insts[name]) if i.startswith("s_barrier")) < first_end, name
