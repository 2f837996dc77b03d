"""Guards on the generated gfx950 code (CPU: hipcc cross-compiles; no GPU needed).

ROCm 7.2's hipcc can turn two "shift right, clamp to 0..255" results packed into one word into V_ASHR_PK_U8_I32 and OR
further bytes in above bit 16 -- but the MI355X keeps bits 31:16 of that instruction's destination, so the word is
wrong (tests/cases/ashr_pk_u8.hip shows it on the GPU; DESIGN.md "Toolchain cases").  k_warp_split4 carries a register
barrier against it.  This test compiles every kernel file to assembly and fails if the instruction (or its signed
sibling) appears anywhere in the product, i.e. if a future edit or toolchain re-introduces the pattern."""
import functools
import glob
import importlib.util
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lane_tracker_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@functools.lru_cache(maxsize=None)
def _isa(path):
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-S",
                        "--cuda-device-only", "-I", CSRC, path, "-o", "-"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_no_packed_clamp_shift_instruction_in_the_product():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert files
    with ThreadPoolExecutor(4) as ex:
        listings = list(ex.map(_isa, files))
    for path, text in zip(files, listings):
        hits = [ln.strip() for ln in text.splitlines() if re.search(r"\bv_ashr_pk_[ui]8_i32\b", ln)]
        assert not hits, "%s: %d uses of v_ashr_pk_*8_i32, e.g. %s" % (os.path.basename(path), len(hits), hits[0])
        # the hand-written pieces of the walking threshold kernels must still be there (a guard against silent rewrites)
        if path.endswith("k_threshold_walk.hip"):
            assert "v_cmp_le_i16_e64" in text and "ds_read_b128" in text and "global_load_dwordx4" in text
            assert ".vgpr_spill_count: 0" in text or "vgpr_spill_count:     0" in text
        # the two-row top-hat kernels compare u8 pixels as f16 denormals: every one of them must run with f16 denormals
        # kept (kernel descriptor) and set the mode itself before its first min / max
        if path.endswith("k_tophat.hip"):
            kernels = re.split(r"\n(?=_ZN2lt[^\n]*k_morph_runs2[^\n]*:)", text)[1:]
            assert len(kernels) >= 12
            for k in kernels:
                body = k.split(".end_amdhsa_kernel")[0]
                assert re.search(r"s_setreg_imm32_b32 hwreg\(HW_REG_MODE, 6, 2\), 3", body), k.splitlines()[0]
                assert re.search(r"\.amdhsa_float_denorm_mode_16_64 3", body), k.splitlines()[0]
                assert "scratch_" not in body.split("s_endpgm")[0], k.splitlines()[0]


def _isa_split():
    spec = importlib.util.spec_from_file_location("isa_split", os.path.join(ROOT, "tools", "isa_split.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# DESIGN.md section 4, the budget of the undistortion walks -- the 50 instantiations of k_undistort_rows<LAYOUT, SRC, PER_SLOT>
# (k_frontend.hip), from one compile.  Per layout and source (SRC 0: surfaces, 1 / 2: slots, dword-aligned / at any byte), for both table
# forms: vector-memory instructions (2 table reads, the windows of two tap rows of one frame before the loop and of the next inside it --
# 2 + 2 RGB family and 4:2:2, 4 + 4 NV12 and raw Bayer, 6 + 6 I420 -- and the store); the most v_mul_lo_u32 (quarter rate) it may hold: the
# two of the block-index division in the 3-byte forms, none where a conversion's 24-bit multiplies would be the first to be widened; and
# the most VALU instructions inside the per-frame loop (the compiler's own counts on the finished code, ROCm 7.2, no margin; the 4:2:0
# ones are those of the kernels' former separate bodies, which the shared walk keeps with an empty asm in the blend).  The table-per-slot
# forms have the caps of their one-table peers.
RGB, BAYER = {0: (7, 2, 53), 1: (7, 2, 46), 2: (7, 2, 46)}, {0: (11, 0, 158), 1: (11, 0, 145)}
PER_LAYOUT = {   # layout: {SRC: (vmem, mul_lo, loop VALU)}
    0: RGB,
    1: {0: (11, 0, 148), 1: (11, 0, 134)}, 2: {0: (15, 0, 157), 1: (15, 0, 136)},          # NV12, I420
    3: {0: (7, 0, 114), 1: (7, 0, 107)}, 4: {0: (7, 0, 114), 1: (7, 0, 107)},              # YUY2, UYVY
    5: {s: RGB[s] for s in (0, 1)}, 6: {s: RGB[s] for s in (0, 1)}, 7: {s: RGB[s] for s in (0, 1)},   # BGR, RGBA, BGRA: no more than RGB
    16: BAYER, 17: BAYER, 18: BAYER, 19: BAYER,
}
UNDISTORT_BUDGET = {"k_undistort_rows<%d, %d, %s>" % (layout, src, per_slot): cap
                    for layout, by_src in PER_LAYOUT.items() for src, cap in by_src.items() for per_slot in ("false", "true")}


@functools.lru_cache(maxsize=None)
def _walks():
    """-> (name -> counts, name -> instructions) of the walks, from the one compile of k_frontend.hip."""
    split, isa = _isa_split(), _isa(os.path.join(CSRC, "k_frontend.hip"))
    return split.table(isa, "k_undistort_rows"), {split.kernel_name(n): k["insts"] for n, k in split.kernels(isa).items()}


def _hold(layouts, per_slot=("false", "true")):
    """The walks of `layouts` in the table forms `per_slot` against their rows of the table -> [(name, counts)], for what a family adds."""
    table, held = _walks()[0], []
    for name, (vmem, mul_lo, loop_valu) in UNDISTORT_BUDGET.items():
        if int(name[name.index("<") + 1:name.index(",")]) not in layouts or name[name.rindex(" ") + 1:-1] not in per_slot:
            continue
        st = table[name]
        print(name, st)
        assert st["vmem"] == vmem, "%s: %d vector-memory instructions, budget %d" % (name, st["vmem"], vmem)
        assert st["mul_lo"] <= mul_lo, "%s: %d v_mul_lo_u32, budget %d" % (name, st["mul_lo"], mul_lo)
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["loop_valu"] is not None, "%s: no per-frame loop found" % name
        assert st["loop_valu"] <= loop_valu, "%s: %d VALU instructions per frame, budget %d" % (name, st["loop_valu"], loop_valu)
        held.append((name, st))
    return held


needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


@needs_hipcc
def test_undistortion_walks_keep_their_instruction_budget():
    """The table lists exactly the walks that exist; RGB's one-table forms and 4:2:0's forms, one table and table per slot."""
    assert len(UNDISTORT_BUDGET) == 50 and sorted(_walks()[0]) == sorted(UNDISTORT_BUDGET), sorted(_walks()[0])
    assert len(_hold({0}, ("false",))) == 3 and len(_hold({1, 2})) == 8


@needs_hipcc
def test_rgb_table_per_slot_forms_keep_the_caps_of_the_one_table_forms():
    assert len(_hold({0}, ("true",))) == 3


@needs_hipcc
def test_rgb_family_instantiations_cost_no_more_than_rgb():
    assert len(_hold({5, 6, 7})) == 12


@needs_hipcc
def test_422_instantiations_keep_their_budget_and_eight_waves():
    held = _hold({3, 4})
    assert len(held) == 8
    for name, st in held:                    # no quarter-rate multiply at all, and eight waves per SIMD
        assert st["mul_lo"] == 0, "%s: %d v_mul_lo_u32" % (name, st["mul_lo"])
        assert st["vgpr"] < 64, "%s: %d VGPRs" % (name, st["vgpr"])


@needs_hipcc
def test_bayer_instantiations_keep_their_counts_and_load_whole_dwords():
    held = _hold({16, 17, 18, 19})
    assert len(held) == 16
    for name, _ in held:
        # every window is the aligned dwords that hold it: no byte or short loads from the frames (the 16-bit loads are the two
        # remap-table reads)
        loads = [i for i in _walks()[1][name] if re.match(r"^(buffer|global|flat)_load", i)]
        assert not any("ubyte" in i or "sbyte" in i for i in loads), (name, loads)
        assert sum("buffer_load_dwordx2" in i for i in loads) == 8, (name, loads)
