#!/usr/bin/env python3
"""Host-fed throughput with RGB and with NV12 camera frames: what the halved bus bytes of YUV 4:2:0 input buy.

Legs, at 1280x720 and 1920x1080, for pixel formats 'rgb' and 'nv12' (frames from ordinary host memory, a drifting synthetic
lane with a short outage; the NV12 frames are the RGB ones converted on the CPU beforehand, outside the timed region):
  batch            process_batch(256 frames, annotate=False)                     frames/s
  stream           process_stream(windows of 128 frames, annotate=False)         frames/s
  stream_annotated process_stream(windows of 128 frames, annotate=True)          frames/s
  process          process() frame by frame, annotated                           frames/s
Every leg runs `--runs` times (default 3); the file holds each run, the median and the range, and the commit hash.

The RGB legs use nothing newer than `LaneTracker(...)`, `process()`, `process_batch()` and `process_stream()`, so this file runs
unchanged on a checkout that has no 4:2:0 input (its NV12 legs are skipped and say so): the yardstick for the NV12 figures is the
RGB figure of the same leg from such a checkout on the same machine.

  python tools/yuv_input_bench.py [--runs 3] [--out profiles/yuv_input.json] [--sizes 1280x720,1920x1080] [--formats rgb,nv12] [--commit HASH]
"""
import argparse
import inspect
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lane_tracker_amd import calib, synth  # noqa: E402
from lane_tracker_amd.lane_tracker import LaneTracker  # noqa: E402

HAS_YUV = "pixel_format" in inspect.signature(LaneTracker.__init__).parameters
POOL = 32


def rgb_to_nv12(rgb):
    """BT.601 video range, chroma the mean of each 2 x 2 block (only makes inputs)."""
    f = rgb.astype(np.float32)
    h, w = f.shape[:2]
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 0.257 * r + 0.504 * g + 0.098 * b + 16
    u = -0.148 * r - 0.291 * g + 0.439 * b + 128
    v = 0.439 * r - 0.368 * g - 0.071 * b + 128
    mean = lambda p: p.reshape(h // 2, 2, w // 2, 2).mean((1, 3))
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    return np.concatenate([q(y), np.stack([q(mean(u)), q(mean(v))], -1).reshape(h // 2, w)])


def frames_for(cal, fmt, n):
    pool = synth.stream_lanes(POOL, seed=5, cal=cal).copy()
    pool[20:23] = 0                     # a short outage: second tries, failure pictures
    if fmt == "nv12":
        pool = np.stack([rgb_to_nv12(f) for f in pool])
    return np.ascontiguousarray(pool[np.arange(n) % POOL])


def tracker(cal, fmt):
    return LaneTracker(**cal) if fmt == "rgb" else LaneTracker(**cal, pixel_format=fmt)


def leg_batch(cal, fmt, frames):
    t = tracker(cal, fmt)
    try:
        t.process_batch(frames[:64], annotate=False)            # buffers, code objects
        t0 = time.perf_counter()
        t.process_batch(frames, annotate=False)
        return len(frames) / (time.perf_counter() - t0)
    finally:
        t.close()


def leg_stream(cal, fmt, frames, annotate, windows=6, size=128):
    t = tracker(cal, fmt)
    try:
        wins = [frames[:size]] * (windows + 1)
        n, t0 = 0, None
        for k, out in enumerate(t.process_stream(wins, annotate=annotate)):
            if k == 0:                                           # the first window pays the set-up
                t0 = time.perf_counter()
            else:
                n += len(out)
        return n / (time.perf_counter() - t0)
    finally:
        t.close()


def leg_process(cal, fmt, frames, n=150, warm=20):
    t = tracker(cal, fmt)
    try:
        for k in range(warm):
            t.process(frames[k % len(frames)])
        t0 = time.perf_counter()
        for k in range(n):
            t.process(frames[(warm + k) % len(frames)])
        return n / (time.perf_counter() - t0)
    finally:
        t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_input.json"))
    ap.add_argument("--sizes", default="1280x720,1920x1080")
    ap.add_argument("--formats", default="rgb,nv12")
    ap.add_argument("--legs", default="batch,stream,stream_annotated,process")
    ap.add_argument("--commit", default=None, help="the commit hash to record (default: git rev-parse HEAD of this checkout)")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = None
    cals = {"1280x720": calib.reference_calibration, "1920x1080": lambda: calib.scaled_calibration(1.5)}
    result = dict(tool="yuv_input_bench", commit=commit, has_yuv_input=HAS_YUV, runs=a.runs, legs=[])
    for size in a.sizes.split(","):
        cal = cals[size]()
        for fmt in a.formats.split(","):
            if fmt != "rgb" and not HAS_YUV:
                result["legs"].append(dict(size=size, pixel_format=fmt, skipped="this checkout has no 4:2:0 input"))
                print(json.dumps(result["legs"][-1]), flush=True)
                continue
            frames = frames_for(cal, fmt, 256)
            w, h = cal["img_size"]
            for leg in a.legs.split(","):
                fn = {"batch": lambda: leg_batch(cal, fmt, frames), "stream": lambda: leg_stream(cal, fmt, frames, False),
                      "stream_annotated": lambda: leg_stream(cal, fmt, frames, True), "process": lambda: leg_process(cal, fmt, frames)}[leg]
                fps = [round(fn(), 1) for _ in range(a.runs)]
                line = dict(size=size, pixel_format=fmt, leg=leg, fps=fps, median=float(np.median(fps)), lo=min(fps), hi=max(fps),
                            bus_bytes_per_row=(3 * w if fmt == "rgb" else 3 * w // 2))
                result["legs"].append(line)
                print(json.dumps(line), flush=True)
    if a.out and a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
