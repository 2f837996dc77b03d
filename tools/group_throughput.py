#!/usr/bin/env python3
"""LaneTrackerGroup throughput against K solo trackers: one JSON line per (size, K).

For K streams of synthetic video (synth.stream_lanes with an outage of black frames, each stream at its own phase of a shared
pool of frames), annotated, process()'s default keywords:
  group_fps        K * ticks / seconds of LaneTrackerGroup.process() over `--ticks` ticks (after `--warmup`)
  tick_ms_median / tick_ms_p99
  solo_fps         K LaneTrackers stepped round-robin from one thread, the same frames (K * ticks / seconds)
  group_cpu_s_per_frame / solo_cpu_s_per_frame   process CPU time (user + system, resource.getrusage) per frame
  vs_one_solo      group_fps / the K = 1 solo rate of the same size (the rate of ONE LaneTracker.process() stream)

  python tools/group_throughput.py [--ticks 60] [--warmup 8] [--out profiles/group_throughput.jsonl] [--no-solo]
"""
import argparse
import json
import os
import resource
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lane_tracker_amd import LaneTrackerGroup, calib, synth  # noqa: E402
from lane_tracker_amd.lane_tracker import LaneTracker  # noqa: E402

POOL = 64


def pool_frames(cal):
    f = synth.stream_lanes(POOL, seed=5, cal=cal).copy()
    f[40:46] = 0                        # an outage: second tries, then sliding windows again
    return f


def cpu_s():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def tick_frames(pool, k, t):
    return [pool[(t + 11 * i) % POOL] for i in range(k)]


def run_group(cal, pool, k, ticks, warmup):
    with LaneTrackerGroup(k, **cal) as g:
        for t in range(warmup):
            g.process(tick_frames(pool, k, t))
        times = []
        c0, t0 = cpu_s(), time.perf_counter()
        for t in range(warmup, warmup + ticks):
            a = time.perf_counter()
            g.process(tick_frames(pool, k, t))
            times.append(time.perf_counter() - a)
        wall, cpu = time.perf_counter() - t0, cpu_s() - c0
    return wall, cpu, np.array(times)


def run_solo(cal, pool, k, ticks, warmup):
    ts = [LaneTracker(**cal) for _ in range(k)]
    try:
        for t in range(warmup):
            for i, f in enumerate(tick_frames(pool, k, t)):
                ts[i].process(f)
        c0, t0 = cpu_s(), time.perf_counter()
        for t in range(warmup, warmup + ticks):
            for i, f in enumerate(tick_frames(pool, k, t)):
                ts[i].process(f)
        return time.perf_counter() - t0, cpu_s() - c0
    finally:
        for t in ts:
            t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--ks-1080p", default="1,8")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--no-solo", action="store_true", help="the group only (a kernel trace of the group's ticks)")
    a = ap.parse_args()
    plan = [("1280x720", calib.reference_calibration(), [int(v) for v in a.ks.split(",") if v]),
            ("1920x1080", calib.scaled_calibration(1.5), [int(v) for v in a.ks_1080p.split(",") if v])]
    out = open(a.out, "a") if a.out else None
    for size, cal, ks in plan:
        pool = pool_frames(cal)
        one_solo = None
        for k in ks:
            gw, gc, times = run_group(cal, pool, k, a.ticks, a.warmup)
            n = k * a.ticks
            sw, sc = run_solo(cal, pool, k, a.ticks, a.warmup) if not a.no_solo else (float("nan"), float("nan"))
            solo_fps = n / sw
            if k == 1:
                one_solo = solo_fps
            line = dict(tool="group_throughput", size=size, k=k, ticks=a.ticks, group_fps=round(n / gw, 1),
                        tick_ms_median=round(float(np.median(times)) * 1e3, 3), tick_ms_p99=round(float(np.percentile(times, 99)) * 1e3, 3),
                        solo_fps=round(solo_fps, 1), group_cpu_s_per_frame=round(gc / n, 6), solo_cpu_s_per_frame=round(sc / n, 6),
                        vs_one_solo=None if one_solo is None else round(n / gw / one_solo, 2))
            s = json.dumps(line)
            print(s, flush=True)
            if out:
                out.write(s + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
