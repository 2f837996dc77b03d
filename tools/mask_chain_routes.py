#!/usr/bin/env python3
"""Every row of the mask chain's route table once, through _native.Context -- the program a kernel trace of
the chain is taken from (rocprofv3 --kernel-trace --stats -- python tools/mask_chain_routes.py), so that two builds of the
library can be compared launch by launch (LANE_TRACKER_AMD_LIB selects the build; tools/mask_chain_compare.py compares).

  mask_chain_routes.py                the rows, one line each: what was asked and which route the library reports
  mask_chain_routes.py --mask-step N  instead: N timed 256-frame mask steps (resident frames, default parameters), us per step
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lane_tracker_amd import _native, calib, synth

WALK_FRAMES = 96        # above walk_min_pixels (80 frames of 1100 x 1080)


def context(cal, capacity):
    return _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                           device=0, capacity=capacity)


def row(c, label, frames, **kw):
    n = len(frames)
    c.upload_frames(frames)
    c.mask_run(n, _native.filter_params(**kw))
    c.sync()
    ones = int(c.download_masks(n).astype(bool).sum())
    print("%-58s frames %3d  threshold_path %2d  adaptive_path %2d  open_form %2d  mask pixels %d" %
          (label, n, c.last_threshold_path(), c.last_adaptive_path(), c.last_open_form(), ones), flush=True)


def routes():
    cal = calib.reference_calibration()
    r = synth.SceneRenderer()
    base = np.stack([r.render(40 + i)[0] for i in range(4)], 0)
    take = lambda n: base[np.arange(n) % len(base)]
    c = context(cal, 2)                      # process()'s context: one and two frames per call
    row(c, "one frame, defaults", take(1))
    row(c, "two frames, defaults", take(2))
    c.close()
    c = context(cal, WALK_FRAMES)
    row(c, "8 frames, defaults", take(8))
    row(c, "21 frames, windows 25 / 31", take(21), ksize_r=25, C_r=6, ksize_b=31, C_b=4)
    row(c, "batch above walk_min_pixels, defaults", take(WALK_FRAMES))
    row(c, "batch above walk_min_pixels, mask_noise", take(WALK_FRAMES), mask_noise=True)
    row(c, "21 frames, neighborhood with its greenery mask", take(21), filter_type="neighborhood", C_r=5, mask_noise=True, noise_thresh=120)
    row(c, "21 frames, neighborhood", take(21), filter_type="neighborhood", C_r=5)
    c.close()
    # the odd-width geometry of tests/test_gpu_parity.py::test_odd_sizes_take_the_generic_paths
    S = np.diag([0.5, 0.5, 1.0])
    c = _native.Context((641, 361), (541, 551), S @ calib.CAM_MATRIX, calib.DIST_COEFFS, S @ calib.M @ np.diag([2.0, 2.0, 1.0]), device=0, capacity=3)
    odd = np.random.default_rng(12).integers(0, 256, (3, 361, 641, 3), dtype=np.uint8)
    row(c, "odd width 541 x 551, defaults", odd)
    row(c, "odd width 541 x 551, neighborhood", odd, filter_type="neighborhood", C_r=5)
    row(c, "odd width 541 x 551, mask_noise", odd, mask_noise=True)
    bev = np.random.default_rng(5).integers(0, 256, (132, 184, 3), dtype=np.uint8)
    for label, kw in (("bilateral", {}), ("bilateral, mask_noise", dict(mask_noise=True)), ("neighborhood", dict(filter_type="neighborhood", C_r=5))):
        m = c.filter_lane_points(bev, _native.filter_params(**kw))
        print("%-58s mask pixels %d  live bytes %d" % ("filter_lane_points 132 x 184, " + label, int(m.astype(bool).sum()),
                                                       _native.device_cache_stats()["live_bytes"]), flush=True)
    c.close()


def mask_step(steps):
    cal = calib.reference_calibration()
    r = synth.SceneRenderer()
    base = np.stack([r.render(40 + i)[0] for i in range(8)], 0)
    c = context(cal, 256)
    c.upload_frames(base[np.arange(256) % 8])
    for _ in range(5):
        c.mask_run(256)
    c.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        c.mask_run(256)
    c.sync()
    print("mask step of 256 frames: %.1f us" % ((time.perf_counter() - t0) / steps * 1e6), flush=True)
    c.close()


if __name__ == "__main__":
    if "--mask-step" in sys.argv:
        mask_step(int(sys.argv[sys.argv.index("--mask-step") + 1]))
    else:
        routes()
