#!/usr/bin/env python3
"""The threshold stage on a batch in which every tile is live: what the dead-tile test of k_threshold_mma.hip costs when it saves nothing.

    python tools/threshold_skip_worstcase.py [--frames 256] [--steps 5] [--reps 3]

256 resident bird's-eye frames of uniform noise (eight distinct ones, repeated) go through lt_filter_run on one stream with the
stage timers on; the line printed is {"threshold_ms": [one figure per repetition, ms per step], "live_share_h", "live_share_v"}.
The live shares are asserted to be 1.0 on the oracle's top-hat planes of one of the frames, in the kernel's tiling (32 x 32 and
32 x 128), for both planes and their C.  Which build runs is the caller's choice: LANE_TRACKER_AMD_LIB names another library (the
parent's, or the experiments build with LT_THRESHOLD_SKIP=0); take the figures of the builds in turns in one sitting."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tile_max(plane, th, tw):
    h, w = plane.shape
    return np.array([[plane[y:y + th, x:x + tw].max() for x in range(0, w, tw)] for y in range(0, h, th)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from lane_tracker_amd import _native, calib
    from oracle import oracle as O
    cal = calib.reference_calibration()
    w, h = cal["warped_size"]
    rng = np.random.default_rng(2024)
    distinct = rng.integers(0, 256, (8, h, w, 3), dtype=np.uint8)
    fp, ofp = _native.filter_params(), O.filter_params()
    planes = O.filter_lane_points(distinct[0], ofp, want_planes=True)[1]
    shares = {}
    for name, (th, tw) in (("live_share_h", (32, 32)), ("live_share_v", (32, 128))):
        shares[name] = min(float((tile_max(planes[2], th, tw) > fp.C_r).mean()), float((tile_max(planes[3], th, tw) > fp.C_b).mean()))
        assert shares[name] == 1.0, shares

    ctx = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                          device=0, capacity=a.frames)
    try:
        for c0 in range(0, a.frames, 8):
            ctx.upload_bev(distinct[:min(8, a.frames - c0)], first=c0)
        ctx.set_streams(1)
        ctx.filter_run(a.frames, fp)                        # warm-up
        ctx.sync()
        assert ctx.last_threshold_form() == 2
        ctx.set_stage_timing(True)
        series = []
        for _ in range(a.reps):
            ctx.stage_reset()
            for _ in range(a.steps):
                ctx.filter_run(a.frames, fp)
            ctx.sync()
            series.append(round(ctx.stage_ms()["threshold"][0] / a.steps, 4))
        print(json.dumps(dict(shares, threshold_ms=series, frames=a.frames, lib=os.path.basename(_native.LIB_PATH),
                              skip_env=os.environ.get("LT_THRESHOLD_SKIP"))))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
