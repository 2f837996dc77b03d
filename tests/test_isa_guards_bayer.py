"""Guards on the generated gfx950 code of the raw Bayer undistortion walks (CPU: hipcc cross-compiles; no GPU needed): the sixteen
entry points of `undistort_walk` for the four patterns -- slots, surfaces, and the table-per-slot forms of both -- counted by
tools/isa_split.py as the RGB, 4:2:0, 4:2:2 and RGB-family forms are.  A frame costs four window loads, as NV12 does; no byte
loads, no quarter-rate multiply, no scratch; the demosaic of the four taps stays inside its VALU count."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lane_tracker_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (vector-memory instructions, v_mul_lo_u32, VALU instructions inside the per-frame loop).  Vector memory: 2 table reads, the 4 windows
# of the first frame before the loop and the 4 of the next inside it, 1 store -- NV12's 11 (tests/test_isa_guards.py).  VALU: counted
# on the commit that added the format (ROCm 7.2), no margin; NV12 has 110 / 124:
#       hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -S --cuda-device-only -I lane_tracker_amd/csrc \
#             lane_tracker_amd/csrc/k_frontend.hip -o k_frontend.s && python tools/isa_split.py k_frontend.s --match k_undistort_bayer
SLOT, SURF = (11, 0, 145), (11, 0, 158)
CAPS = {}
for _p in range(4):
    CAPS["k_undistort_bayer<%d>" % _p] = SLOT
    CAPS["k_undistort_bayer_cal<%d>" % _p] = SLOT
    CAPS["k_undistort_bayer_surf<%d>" % _p] = SURF
    CAPS["k_undistort_bayer_cal_surf<%d>" % _p] = SURF


def _isa_split():
    spec = importlib.util.spec_from_file_location("isa_split", os.path.join(ROOT, "tools", "isa_split.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                        "-I", CSRC, os.path.join(CSRC, "k_frontend.hip"), "-o", "-"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_bayer_walks_keep_their_counts(isa):
    split = _isa_split()
    table = split.table(isa, "k_undistort_bayer")
    assert sorted(table) == sorted(CAPS), sorted(table)
    for name, (vmem, mul_lo, loop_valu) in CAPS.items():
        st = table[name]
        print(name, st)
        assert st["vmem"] == vmem, "%s: %d vector-memory instructions, budget %d" % (name, st["vmem"], vmem)
        assert st["mul_lo"] <= mul_lo, "%s: %d v_mul_lo_u32" % (name, st["mul_lo"])
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["loop_valu"] is not None, "%s: no per-frame loop found" % name
        assert st["loop_valu"] <= loop_valu, "%s: %d VALU instructions per frame, budget %d" % (name, st["loop_valu"], loop_valu)
    # every window is the aligned dwords that hold it: the walks issue no byte or short loads from the frames (the 16-bit loads are
    # the two remap-table reads)
    ks = split.kernels(isa)
    walks = [k for k in ks if "k_undistort_bayer" in k]
    assert len(walks) == 16
    for k in walks:
        loads = [i for i in ks[k]["insts"] if re.match(r"^(buffer|global|flat)_load", i)]
        assert not any("ubyte" in i or "sbyte" in i for i in loads), (k, loads)
        assert sum("buffer_load_dwordx2" in i for i in loads) == 8, (k, loads)
