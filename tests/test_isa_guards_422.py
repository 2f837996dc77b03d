"""Guards on the generated gfx950 code of the packed 4:2:2 undistortion walks (CPU: hipcc cross-compiles; no GPU needed): the
eight entry points of `undistort_walk` for YUY2 / UYVY -- slots, surfaces, and the table-per-slot forms of both -- keep the
instruction budget DESIGN.md section 4 states for them, counted by tools/isa_split.py as for the RGB and 4:2:0 forms."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lane_tracker_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel: the most VALU instructions inside the per-frame loop -- the compiler's own count on the finished code (ROCm 7.2), below the
# NV12 forms' 134 (slots) / 148 (surfaces): two windows instead of four, and a select per tap instead of a second shift
LOOP_VALU = {
    "k_undistort422<0>": 107, "k_undistort422<1>": 107,
    "k_undistort422_cal<0>": 107, "k_undistort422_cal<1>": 107,
    "k_undistort422_surf<0>": 114, "k_undistort422_surf<1>": 114,
    "k_undistort422_cal_surf<0>": 114, "k_undistort422_cal_surf<1>": 114,
}


def _isa_split():
    spec = importlib.util.spec_from_file_location("isa_split", os.path.join(ROOT, "tools", "isa_split.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_422_undistortion_walks_keep_their_instruction_budget():
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                        "-I", CSRC, os.path.join(CSRC, "k_frontend.hip"), "-o", "-"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    table = _isa_split().table(r.stdout, "k_undistort422")
    assert sorted(table) == sorted(LOOP_VALU), sorted(table)
    assert not any("k_undistort_rows" in name for name in table)     # (the existing guard counts the kernels of that name: its seven)
    for name, loop_valu in LOOP_VALU.items():
        st = table[name]
        print(name, st)
        # 2 table reads, 2 windows of the first frame before the loop and 2 of the next inside it, 1 store
        assert st["vmem"] == 7, "%s: %d vector-memory instructions, budget 7" % (name, st["vmem"])
        assert st["mul_lo"] == 0, "%s: %d v_mul_lo_u32" % (name, st["mul_lo"])
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["vgpr"] < 64, "%s: %d VGPRs" % (name, st["vgpr"])
        assert st["loop_valu"] is not None, "%s: no per-frame loop found" % name
        assert st["loop_valu"] <= loop_valu, "%s: %d VALU instructions per frame, budget %d" % (name, st["loop_valu"], loop_valu)
