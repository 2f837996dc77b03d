"""The split-band form of the batch top-hat walks (csrc/k_tophat.hip: k_morph_split) against the oracle, bit for bit.

A band of the split form walks its own input rows only; the rows within R of a band boundary are merged from the partial
results of the two neighbouring bands through a scratch zone.  The cases are small bird's-eye views cut into FOUR bands (the
experiments build's LT_MORPH_NB_* switches, in a child process, the way test_gpu_parity.py forces its fallbacks):
  (236, 188)  4 bands of 59 rows (odd: band starts are rounded to the walk's rows per trip), a full strip + a 60-column PAIR strip
  (233, 188)  the last band is exactly one 55x55 zone (56 rows)
  (226, 188)  the last band is 55 rows: the 55x55 walk must fall back to the halo form while the 29x29 walk splits
  (236, 256)  no PAIR strip
with 3 frames (the PAIR strip's odd last frame) and 4, on noise and on images whose only bright / dark pixels sit within R rows
of the band boundaries and of rows 0 and h - 1.  `last_tophat_path` tells which form ran.  One child process computes every case
(the GPU planes and the oracle's) once; the tests below read its report."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(ROOT, "lane_tracker_amd", "liblane_tracker_amd_exp.so")

SIZES = [(236, 188), (233, 188), (226, 188), (236, 256)]          # (h, w)
FRAMES = [3, 4]
EXPECT_PATH = {(236, 188): 3, (233, 188): 3, (226, 188): 1, (236, 256): 3}   # bit 0: 29x29 split, bit 1: 55x55 split
NBANDS = 4


def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _boundary_image(rng, h, w, R=27):
    """Mid grey, except for sparse bright and dark pixels within R rows of every band boundary and of rows 0 and h - 1."""
    img = np.full((h, w, 3), 128, np.uint8)
    rows = (h + NBANDS - 1) // NBANDS
    near = np.zeros(h, bool)
    for y in [0, h - 1] + [b * rows for b in range(1, NBANDS)]:
        near[max(y - R, 0):min(y + R + 1, h)] = True
    hit = (rng.random((h, w)) < 0.04) & near[:, None]
    vals = np.where(rng.random((h, w, 1)) < 0.5, rng.integers(0, 40, (h, w, 3)), rng.integers(215, 256, (h, w, 3)))
    img[hit] = vals[hit].astype(np.uint8)
    return img


def _frames(h, w, n):
    rng = np.random.default_rng(h * 1009 + w * 31 + n)
    return np.stack([_noise(rng, h, w) if i % 2 == 0 else _boundary_image(rng, h, w) for i in range(n)], 0)


def _child():
    sys.path.insert(0, ROOT)
    from lane_tracker_amd import _native, calib
    from oracle import oracle as O
    cal = calib.reference_calibration()
    report = {}
    for (h, w) in SIZES:
        for n in FRAMES:
            bev = _frames(h, w, n)
            ctx = _native.Context(cal["img_size"], (w, h), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=n)
            try:
                ctx.set_walk_min_frames(0)       # the padded top-hat planes the walking threshold kernels read, as in a batch
                ctx.upload_bev(bev)
                for noise in (False, True):      # True: the 55x55 top-hat launch also stores its minuend (the greenery mask's plane)
                    kw = dict(mask_noise=True) if noise else {}
                    ctx.filter_run(n, _native.filter_params(**kw))
                    path = ctx.last_tophat_path()
                    masks = ctx.download_masks(n)
                    th_r = ctx.download_plane(_native.PLANE_TOPHAT_R, n)
                    th_b = ctx.download_plane(_native.PLANE_TOPHAT_B, n)
                    bad = {"tophat_r": 0, "tophat_b": 0, "mask": 0}
                    for i in range(n):
                        want, planes = O.filter_lane_points(bev[i], O.filter_params(**kw), want_planes=True)
                        bad["tophat_r"] += int((th_r[i] != planes[2]).sum())
                        bad["tophat_b"] += int((th_b[i] != planes[3]).sum())
                        bad["mask"] += int((masks[i] != want).sum())
                    report["%d,%d,%d,%d" % (h, w, n, int(noise))] = dict(path=path, **bad)
            finally:
                ctx.close()
    print("REPORT " + json.dumps(report))


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(EXP_LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "lane_tracker_amd", "csrc"), "-s", "-j8", "EXPERIMENTS=1"])
    env = dict(os.environ, LANE_TRACKER_AMD_LIB=EXP_LIB)
    for name in ("LT_MORPH_NB_29E", "LT_MORPH_NB_29D", "LT_MORPH_NB_55E", "LT_MORPH_NB_55D"):
        env[name] = str(NBANDS)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=ROOT, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("REPORT ")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(line[-1][len("REPORT "):])


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("n", FRAMES)
@pytest.mark.parametrize("size", SIZES)
def test_split_band_walks_are_bit_exact(report, size, n, noise):
    h, w = size
    got = report["%d,%d,%d,%d" % (h, w, n, int(noise))]
    print(size, n, noise, got)
    assert got["path"] == EXPECT_PATH[size], "the top-hat walks did not take the expected form"
    assert got["tophat_r"] == 0, "29x29 top-hat of the R plane differs from the oracle"
    assert got["tophat_b"] == 0, "55x55 top-hat of the Lab-b plane differs from the oracle"
    assert got["mask"] == 0, "mask differs from the oracle"


if __name__ == "__main__" and "--child" in sys.argv:
    _child()
