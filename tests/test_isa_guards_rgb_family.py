"""Guards on the generated gfx950 code of the BGR / RGBA / BGRA undistortion walks (CPU: hipcc cross-compiles; no GPU needed): the
twelve entry points of `undistort_walk` for layouts 5, 6 and 7 -- slots, surfaces, and the table-per-slot forms of both -- cost no
more than their RGB peers, counted by tools/isa_split.py as for the RGB, 4:2:0 and 4:2:2 forms.  A permuted channel order is another
constant in a shift the walk already has; a 4-byte pixel is a select per tap instead of a 64-bit shift."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lane_tracker_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# The caps are the RGB peers' own counts: (vector-memory instructions, v_mul_lo_u32, VALU instructions inside the per-frame loop).
#   slots / surfaces: k_undistort_rows<true> (7, 2, 46) / k_undistort_rows_surf (7, 2, 53) -- tests/test_isa_guards.py
#   table per slot:   k_undistort_cal<true> (7, 2, 46) / k_undistort_cal_surf (7, 2, 53) -- measured on the commit before this one
#                     (ROCm 7.2), no margin:
#       hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -S --cuda-device-only -I lane_tracker_amd/csrc \
#             lane_tracker_amd/csrc/k_frontend.hip -o k_frontend.s && python tools/isa_split.py k_frontend.s k_undistort_cal
SLOT, SURF = (7, 2, 46), (7, 2, 53)
CAPS = {}
for _f in (5, 6, 7):
    CAPS["k_undistort_px<%d>" % _f] = SLOT
    CAPS["k_undistort_px_cal<%d>" % _f] = SLOT
    CAPS["k_undistort_px_surf<%d>" % _f] = SURF
    CAPS["k_undistort_px_cal_surf<%d>" % _f] = SURF
# ... and the RGB table-per-slot forms themselves, which no other guard counts
RGB_CAL = {"k_undistort_cal<true>": SLOT, "k_undistort_cal<false>": SLOT, "k_undistort_cal_surf": SURF}


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


def _check(table, caps):
    for name, (vmem, mul_lo, loop_valu) in caps.items():
        st = table[name]
        print(name, st)
        # 2 table reads, 2 windows of the first frame before the loop and 2 of the next inside it, 1 store
        assert st["vmem"] == vmem, "%s: %d vector-memory instructions, budget %d" % (name, st["vmem"], vmem)
        assert st["mul_lo"] <= mul_lo, "%s: %d v_mul_lo_u32, its RGB peer has %d" % (name, st["mul_lo"], mul_lo)
        assert st["scratch"] == 0, "%s uses scratch" % name
        assert st["loop_valu"] is not None, "%s: no per-frame loop found" % name
        assert st["loop_valu"] <= loop_valu, "%s: %d VALU instructions per frame, its RGB peer has %d" % (name, st["loop_valu"], loop_valu)


def test_rgb_family_walks_cost_no_more_than_rgb(isa):
    table = _isa_split().table(isa, "k_undistort_px")
    assert sorted(table) == sorted(CAPS), sorted(table)
    # (the existing guards count the kernels of these names: their seven and their eight)
    assert not any("k_undistort_rows" in name or "k_undistort422" in name for name in table)
    _check(table, CAPS)


def test_rgb_table_per_slot_walks_keep_their_counts(isa):
    table = _isa_split().table(isa, "k_undistort_cal")
    _check(table, RGB_CAL)
