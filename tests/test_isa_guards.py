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


# DESIGN.md section 4, the budget of the undistortion walks: vector-memory instructions per kernel (table read 2, two tap rows of one
# frame before the loop and of the next inside it -- 2 + 2 windows RGB, 4 + 4 NV12, 6 + 6 I420 -- and the store); the most
# v_mul_lo_u32 (quarter rate) it may hold: the two of the block-index division in the RGB forms, none where the 4:2:0 conversion's
# 24-bit multiplies would be the first to be widened; and the most VALU instructions inside the per-frame loop (the counts of the
# kernels' former separate bodies, which the shared walk keeps with an empty asm in the blend: k_frontend.hip).
UNDISTORT_BUDGET = {   # kernel: (vmem, mul_lo, loop VALU)
    "k_undistort_rows<true>": (7, 2, 46),
    "k_undistort_rows<false>": (7, 2, 46),
    "k_undistort_rows_surf": (7, 2, 53),
    "k_undistort_rows_yuv<1>": (11, 0, 134),
    "k_undistort_rows_yuv<2>": (15, 0, 136),
    "k_undistort_rows_yuv_surf<1>": (11, 0, 148),
    "k_undistort_rows_yuv_surf<2>": (15, 0, 157),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_undistortion_walks_keep_their_instruction_budget():
    table = _isa_split().table(_isa(os.path.join(CSRC, "k_frontend.hip")), "k_undistort_rows")
    assert sorted(table) == sorted(UNDISTORT_BUDGET), sorted(table)
    for name, (vmem, mul_lo, loop_valu) in UNDISTORT_BUDGET.items():
        st = table[name]
        print(name, st)
        assert st["vmem"] == vmem, "%s: %d vector-memory instructions, budget %d" % (name, st["vmem"], vmem)
        assert st["mul_lo"] <= mul_lo, "%s: %d v_mul_lo_u32, budget %d" % (name, st["mul_lo"], mul_lo)
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["loop_valu"] is not None, "%s: no per-frame loop found" % name
        assert st["loop_valu"] <= loop_valu, "%s: %d VALU instructions per frame, budget %d" % (name, st["loop_valu"], loop_valu)
