"""Guards on the generated gfx950 code of the split-band top-hat walks (CPU: hipcc cross-compiles; no GPU needed).

k_morph_split (csrc/k_tophat.hip) runs the row loop of k_morph_runs2 plus a zone prologue, one barrier and a merging tail.  The
walks are bound by VALU issue and the LDS pipe at 4 (55x55) and 5 (29x29) waves per SIMD, so each new instantiation must keep the
occupancy step of the k_morph_runs2 kernel it replaces, spill nothing, and run with f16 denormals kept (the u8 pixels are compared
as f16 denormals).  All of it is read from the metadata and kernel descriptors hipcc writes."""
import functools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lane_tracker_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


@functools.lru_cache(maxsize=None)
def _listing():
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                        "-I", CSRC, os.path.join(CSRC, "k_tophat.hip"), "-o", "-"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _metadata():
    """mangled kernel name -> dict of the integer fields of its amdhsa.kernels entry"""
    text = _listing()
    md = text[text.index("amdhsa.kernels:"):]
    out = {}
    for entry in re.split(r"\n\s+- \.agpr_count", md)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*\n", entry)}
    return out


def _waves_per_simd(vgprs):
    """gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves"""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def _flags(mangled):
    return re.findall(r"Lb([01])E", mangled.split("EEvPKh")[0] + "E")   # the template's bool arguments, in order


def test_split_kernels_keep_occupancy_spill_nothing_and_keep_f16_denormals():
    md = _metadata()
    split = {n: m for n, m in md.items() if "k_morph_split" in n}
    runs2 = {n: m for n, m in md.items() if "k_morph_runs2" in n}
    assert len(split) == 7, sorted(split)      # 55x55: erode, dilate, top-hat, top-hat + minuend copy; 29x29: erode, dilate, top-hat
    text = _listing()
    for name, m in sorted(split.items()):
        se = "SE55" if "SE55" in name else "SE29"
        dil, th, copym = _flags(name)
        # the kernel this one replaces: k_morph_runs2<SE, DIL, WIDE = true, TH, COPYM>
        parent = [p for n, p in runs2.items() if se in n and _flags(n) == [dil, "1", th, copym]]
        assert len(parent) == 1, name
        waves, parent_waves = _waves_per_simd(m["vgpr_count"]), _waves_per_simd(parent[0]["vgpr_count"])
        print(name, "VGPRs", m["vgpr_count"], "waves/SIMD", waves, "| k_morph_runs2:", parent[0]["vgpr_count"], parent_waves)
        assert waves >= parent_waves and waves >= (4 if se == "SE55" else 5), (name, m["vgpr_count"], parent[0]["vgpr_count"])
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        body = text.split("\n" + name + ":")[1].split(".end_amdhsa_kernel")[0]
        assert re.search(r"\.amdhsa_float_denorm_mode_16_64 3", body), name
        assert re.search(r"s_setreg_imm32_b32 hwreg\(HW_REG_MODE, 6, 2\), 3", body), name
        code = body.split("s_endpgm")[0]
        assert "scratch_" not in code, name
        assert len(re.findall(r"\bs_barrier\b", code)) == 2, name   # one per task kind (normal / pair strip): a task crosses ONE barrier
