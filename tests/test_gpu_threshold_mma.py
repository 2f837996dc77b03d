"""The bilateral thresholds as i8 matrix products (csrc/k_threshold_mma.hip) against the NumPy prefix-sum formula and against the
running-sum walks they replace, through the context's own filter chain (lt_upload_bev + lt_filter_run).  `last_threshold_form`
tells which of the two long forms produced the partial planes; `last_threshold_path` keeps saying 1 for both.  The arithmetic is
exact integer arithmetic: every comparison here is for equality."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_walk import _bev, _bilateral_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lane_tracker_amd", "csrc")
EXP_LIB = os.path.join(ROOT, "lane_tracker_amd", "liblane_tracker_amd_exp.so")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (w, h): smaller than every window; one tile and a one-row / four-column remainder; strip and tile remainders; one row past a
# 128 group; the two-segment split of each direction; a width of five 128-column trips and a remainder
SIZES = [(8, 5), (36, 33), (64, 64), (132, 70), (128, 129), (72, 650), (1284, 40), (644, 130)]
PARAMS = [(15, 8, 35, 5), (35, 0, 15, 12), (20, 3, 20, 7)]


def _ctx(w, h, capacity=3):
    from lane_tracker_amd import _native, calib
    cal = calib.reference_calibration()
    ctx = _native.Context(cal["img_size"], (w, h), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=capacity)
    ctx.set_walk_min_frames(0)                             # these small calls would take the tile kernel by default
    return ctx


def _images(rng, h, w):
    """-> two runs of three frames: the three image kinds of the walk tests; all 0, all 255, a 0 / 255 checkerboard"""
    yy, xx = np.mgrid[0:h, 0:w]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    return [np.stack([_bev(rng, h, w, k) for k in range(3)], 0),
            np.stack([np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), board], 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_matrix_core_thresholds_match_the_prefix_sum_formula(size):
    from lane_tracker_amd import _native
    from oracle import oracle as O
    w, h = size
    assert w * h < 200000
    ctx = _ctx(w, h)
    rng = np.random.default_rng(w * 104729 + h)
    try:
        for bev in _images(rng, h, w):
            # the oracle's top-hat planes do not depend on the threshold parameters: once per frame
            tophats = [O.filter_lane_points(bev[i], O.filter_params(), want_planes=True)[1][2:4] for i in range(3)]
            for kr, cr, kb, cb in PARAMS:
                ctx.upload_bev(bev)
                ctx.filter_run(3, _native.filter_params(ksize_r=kr, C_r=cr, ksize_b=kb, C_b=cb))
                assert ctx.last_threshold_form() == 2, "the matrix-core form did not take these parameters"
                assert ctx.last_threshold_path() == 1
                got = ctx.download_masks(3)
                merged = ctx.download_plane(_native.PLANE_MERGED, 3)
                for i in range(3):
                    tag = (size, (kr, cr, kb, cb), i)
                    expect = _bilateral_np(tophats[i][0], kr, cr) | _bilateral_np(tophats[i][1], kb, cb)
                    diff = (merged[i] > 0) != expect
                    assert not diff.any(), (tag, int(diff.sum()), np.argwhere(diff)[:4].tolist())
                    want = O.filter_lane_points(bev[i], O.filter_params(ksize_r=kr, C_r=cr, ksize_b=kb, C_b=cb))
                    assert np.array_equal(got[i], want), tag
                    assert np.array_equal(got[i] > 0, O.morph_open(expect.astype(np.uint8) * 255, 5) > 0), tag
    finally:
        ctx.close()


_CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
from lane_tracker_amd import _native, calib
from test_gpu_walk import _bev
cal = calib.reference_calibration()
out = {}
for w, h in ((132, 70), (72, 650)):
    ctx = _native.Context(cal["img_size"], (w, h), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=3)
    ctx.set_walk_min_frames(0)
    rng = np.random.default_rng(w * 31 + h)
    bev = np.stack([_bev(rng, h, w, k) for k in range(3)], 0)
    for pi, (kr, cr, kb, cb) in enumerate(((15, 8, 35, 5), (35, 0, 15, 12), (20, 3, 20, 7))):
        ctx.upload_bev(bev)
        ctx.filter_run(3, _native.filter_params(ksize_r=kr, C_r=cr, ksize_b=kb, C_b=cb))
        assert ctx.last_threshold_path() == 1
        assert ctx.last_threshold_form() == int(sys.argv[2]), ctx.last_threshold_form()
        out["merged_%%d_%%d_%%d" %% (w, h, pi)] = ctx.download_plane(_native.PLANE_MERGED, 3)
        out["masks_%%d_%%d_%%d" %% (w, h, pi)] = ctx.download_masks(3)
    ctx.close()
np.savez(sys.argv[1], **out)
print("ok")
'''


@pytest.mark.gpu
def test_matrix_core_form_and_walks_write_identical_planes(tmp_path):
    """One child process per setting of LT_THRESHOLD_MMA with the experiments library: the PLANE_MERGED download and the masks of
    the same inputs are byte-identical between the running-sum walks (0) and the matrix-core form (unset)."""
    if not os.path.exists(EXP_LIB):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8", "EXPERIMENTS=1"])
    code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    files = {}
    for setting, form in (("0", 1), (None, 2)):
        env = dict(os.environ, LANE_TRACKER_AMD_LIB=EXP_LIB)
        env.pop("LT_THRESHOLD_MMA", None)
        if setting is not None:
            env["LT_THRESHOLD_MMA"] = setting
        files[form] = str(tmp_path / ("form%d.npz" % form))
        r = subprocess.run([sys.executable, "-c", code, files[form], str(form)], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
    a, b = np.load(files[1]), np.load(files[2])
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 12
    for name in a.files:
        assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), name


@pytest.mark.gpu
def test_greenery_mask_keeps_its_walk_beside_the_matrix_core_form():
    """mask_noise: form 2 for the two thresholds, the window-65 walk with the range term unchanged, masks equal to the oracle's."""
    from lane_tracker_amd import _native
    from oracle import oracle as O
    w, h = 132, 70
    ctx = _ctx(w, h)
    rng = np.random.default_rng(77)
    try:
        tint, grey = rng.integers(-40, 41, (3, h, w)), rng.integers(60, 200, (3, h, w))       # Lab-b values around the threshold
        for bev in (np.stack([_bev(rng, h, w, k) for k in range(3)], 0),
                    np.clip(np.stack([grey + tint, grey + tint, grey - tint], -1), 0, 255).astype(np.uint8)):
            kw = dict(ksize_r=15, C_r=8, ksize_b=35, C_b=5, mask_noise=True)
            ctx.upload_bev(bev)
            ctx.filter_run(3, _native.filter_params(**kw))
            assert ctx.last_threshold_form() == 2 and ctx.last_threshold_path() == 1
            got = ctx.download_masks(3)
            merged = ctx.download_plane(_native.PLANE_MERGED, 3)
            for i in range(3):
                want, planes = O.filter_lane_points(bev[i], O.filter_params(**kw), want_planes=True)
                noise = ~(planes[1] >= 140) | _bilateral_np(planes[1], 65, 10)
                expect = (_bilateral_np(planes[2], 15, 8) | _bilateral_np(planes[3], 35, 5)) & noise
                assert np.array_equal(merged[i] > 0, expect), i
                assert np.array_equal(got[i], want), i
    finally:
        ctx.close()


@pytest.mark.gpu
def test_other_windows_still_take_the_tile_kernel():
    from lane_tracker_amd import _native
    from oracle import oracle as O
    w, h = 132, 70
    ctx = _ctx(w, h, capacity=1)
    try:
        assert ctx.last_threshold_form() == -1
        bev = _bev(np.random.default_rng(5), h, w, 1)[None]
        kw = dict(ksize_r=17, C_r=8, ksize_b=35, C_b=5)
        ctx.upload_bev(bev)
        ctx.filter_run(1, _native.filter_params(**kw))
        assert ctx.last_threshold_form() == 0 and ctx.last_threshold_path() == 0
        assert np.array_equal(ctx.download_masks(1)[0], O.filter_lane_points(bev[0], O.filter_params(**kw)))
    finally:
        ctx.close()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_generated_code_uses_the_matrix_cores_and_no_scratch():
    """CPU only (hipcc cross-compiles): the i8 32x32x32 MFMA is there, nothing spills, no scratch access before a kernel's end."""
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                        "-I", CSRC, os.path.join(CSRC, "k_threshold_mma.hip"), "-o", "-"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout
    assert "v_mfma_i32_32x32x32_i8" in text
    spills = [ln.strip() for ln in text.splitlines() if ".vgpr_spill_count:" in ln]
    assert spills and all(ln.split(":")[1].strip() == "0" for ln in spills), spills
    for body in text.split(".end_amdhsa_kernel")[:-1]:
        for code in body.split("s_endpgm")[:-1]:
            assert "scratch_" not in code
