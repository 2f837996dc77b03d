#!/usr/bin/env python3
"""Frames per second of the search visualisation and the split view through the stream pipeline (the device paints: lt_search_viz_run /
lt_split_panes_run) beside the only other way to the same images, `process(..., visualize_search=True / split_view=True)` frame by
frame (the host paints in NumPy), on the same machine in the same run.

  process_stream over windows of --window frames of 1280x720 (a drifting lane with a short outage in every 32 frames), annotated,
  --windows of them behind --warmup, wall clock around the generator; process() over --frames frames of the same video.

  python tools/search_viz_rate.py [--window 256] [--windows 6] [--warmup 2] [--frames 48] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lane_tracker_amd import calib, synth  # noqa: E402
from lane_tracker_amd.lane_tracker import LaneTracker  # noqa: E402

POOL = 32


def video(n):
    pool = synth.stream_lanes(POOL, seed=5).copy()
    pool[20:23] = 0                     # a short outage: second tries, bare masks, sliding windows on the way back
    return np.ascontiguousarray(pool[np.arange(n) % POOL])


def stream_rate(window, windows, warmup, **kw):
    lt = LaneTracker(**calib.reference_calibration())
    try:
        win = video(window)
        lt.warm(window, **kw)
        n, t0 = 0, None
        for k, out in enumerate(lt.process_stream((win for _ in range(warmup + windows)), **kw)):
            if k + 1 == warmup:
                t0 = time.perf_counter()
            elif k >= warmup:
                n += len(out)
            del out
        return n / (time.perf_counter() - t0)
    finally:
        lt.close()


def process_rate(frames, **kw):
    lt = LaneTracker(**calib.reference_calibration())
    try:
        vid = video(frames + 4)
        for f in vid[:4]:
            lt.process(f, **kw)
        t0 = time.perf_counter()
        for f in vid[4:]:
            lt.process(f, **kw)
        return frames / (time.perf_counter() - t0)
    finally:
        lt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"window": a.window, "windows": a.windows}
    res["stream_annotated_fps"] = round(stream_rate(a.window, a.windows, a.warmup), 1)        # the rate annotated frames alone travel at
    for name, kw in (("visualize_search", dict(visualize_search=True)), ("split_view", dict(split_view=True))):
        res["stream_%s_fps" % name] = round(stream_rate(a.window, a.windows, a.warmup, **kw), 1)
        res["process_%s_fps" % name] = round(process_rate(a.frames, **kw), 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
