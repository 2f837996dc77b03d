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
                                   [--distinct-calibrations] [--front-end-times]
                                   [--frames-out host|sink|inplace] [--sink-format rgb|nv12|i420] [--device-frames]
  python tools/group_throughput.py --raw-sets [--ks 8,32] [--ticks 40] [--rounds 3] [--out profiles/group_raw_sets.json]

--frames-out: where a tick's annotated frames go -- `host` (the default: one download), `sink` (process(out=) a DeviceFrames of K
surfaces in --sink-format: one lt_overlay_run_to_surfaces per tick) or `inplace` (process(out="inplace"): drawn into the frames
handed in, which must be in device memory).  --device-frames: the inputs of a tick are one-frame DeviceFrames (RGB), refreshed from
the pool before the tick OUTSIDE the timed region; the rates are then K * ticks over the sum of the tick times.  Lines of these
routes carry `frames_out`, `device_frames` and `overlay_launches` (lt_last_overlay_launches after the last tick).

--distinct-calibrations: every stream a camera of its own (stream i: the distortion coefficients x (1 + 0.002 i)), so that the
group's context holds K calibration sets and every slice of a tick mixes them (the table-per-slot front end); `calibrations` in
the line says how many sets the group holds.  --front-end-times: a second, separate pass over the same ticks with the context's
stage timers on (hipEvent pairs around every launch, which also serialise the slices: not for the tick times) -- undistort_ms /
warp_ms per tick, the two front-end launches summed over a tick's slices and tries.

--raw-sets: the raw-sets leg, a run of its own (one JSON document, not lines).  Raw Bayer groups of K cameras (1280 x 720; 8-bit and 12-bit
samples; a table alone, and table + colour stage + shading map), ONE shared raw set (the one-set kernels, fpb frames per walk) against K
distinct ones (every camera its own white-balance gains; with the full setup its own matrix and map too: the set-per-slot kernels).  Both
groups of a cell are alive together and their runs ALTERNATE, --rounds times --ticks ticks each with the stage timers on: undistort_ms per
tick (median over the rounds, and the range), the launches per tick, lt_last_raw_walk_form, and the untimed tick time of a separate pass.
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


def distinct_calibrations(cal, k):
    return [None] + [dict(dist_coeffs=np.asarray(cal["dist_coeffs"], np.float64) * (1.0 + 0.002 * i)) for i in range(1, k)]


class DeviceFeed:
    """The frames of a tick as one-frame DeviceFrames: two sets of K RGB surfaces that take turns (a tick's slots stay attached to
    its surfaces until the tick after the next), filled from the pool before the tick."""

    def __init__(self, cal, k):
        from lane_tracker_amd.device import DeviceFrames
        self.sets = [[DeviceFrames.from_host(np.zeros((cal["img_size"][1], cal["img_size"][0], 3), np.uint8)) for _ in range(k)] for _ in range(2)]

    def tick(self, pool, k, t):
        frames = self.sets[t & 1]
        for f, host in zip(frames, tick_frames(pool, k, t)):
            f.owner.copy_from_host(np.ascontiguousarray(host).reshape(-1))
        return frames

    def close(self):
        for s in self.sets:
            for f in s:
                f.owner.close()


def run_group(cal, pool, k, ticks, warmup, distinct=False, stages=None, frames_out="host", sink_format="nv12", device_frames=False):
    kw = dict(calibrations=distinct_calibrations(cal, k)) if distinct else {}
    feed = DeviceFeed(cal, k) if device_frames else None
    sink = None
    if frames_out == "sink":
        from lane_tracker_amd.device import DeviceFrames
        sink = DeviceFrames.empty(k, cal["img_size"], sink_format)
    pkw = {} if frames_out == "host" else dict(out=sink if frames_out == "sink" else "inplace")
    frames_of = (lambda t: feed.tick(pool, k, t)) if feed else (lambda t: tick_frames(pool, k, t))
    with LaneTrackerGroup(k, **cal, **kw) as g:
        if stages is not None:
            stages["calibrations"] = g.calibration_count() if hasattr(g, "calibration_count") else 1
        for t in range(warmup):
            g.process(frames_of(t), **pkw)
        times = []
        c0, t0 = cpu_s(), time.perf_counter()
        for t in range(warmup, warmup + ticks):
            frames = frames_of(t)
            a = time.perf_counter()
            g.process(frames, **pkw)
            times.append(time.perf_counter() - a)
        wall, cpu = time.perf_counter() - t0, cpu_s() - c0
        if feed:                        # (the refresh of the device frames is not the group's work)
            wall = float(np.sum(times))
        if stages is not None and (pkw or feed):
            stages.update(frames_out=frames_out, device_frames=bool(feed), overlay_launches=g._ctx.last_overlay_launches())
            if sink is not None:
                stages["sink_format"] = sink_format
        if stages is not None and stages.get("front_end"):
            ctx = g._ctx
            ctx.sync()
            ctx.set_stage_timing(True)
            ctx.stage_reset()
            for t in range(warmup + ticks, warmup + 2 * ticks):
                g.process(frames_of(t), **pkw)
            ctx.sync()
            ms = ctx.stage_ms()
            ctx.set_stage_timing(False)
            stages["undistort_ms"] = round(ms["undistort_rows"][0] / ticks, 4)
            stages["warp_ms"] = round(ms["warp_split"][0] / ticks, 4)
            stages["front_end_launches_per_tick"] = round((ms["undistort_rows"][1] + ms["warp_split"][1]) / ticks, 2)
    if feed:
        feed.close()
    if sink is not None and sink.owner is not None:
        sink.owner.close()
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


def raw_sets_leg(a):
    """See the module's docstring: --raw-sets."""
    from lane_tracker_amd import utils
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    rgb = pool_frames(cal)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bayer_reference as RB
    pattern = "bayer_rggb"
    mosaic = RB.rgb_to_bayer(rgb, pattern)
    cells = []
    for bits in (8, 12):
        fmt = pattern if bits == 8 else "bayer12_rggb"
        frames = mosaic if bits == 8 else (mosaic.astype(np.uint16) << 4)
        top = (1 << bits) - 1
        lut = lambda i: utils.raw_lut(0, top, (1.0 + 0.01 * (i % 7), 1, 1.0 + 0.01 * (i % 5)), 1.0, bits=bits)
        ccm = lambda i: utils.raw_ccm(np.eye(3) * (1.0 + 0.001 * i))
        shade = lambda i: utils.raw_shading(np.full((4, 5, 7), 1.0 + 0.002 * i), black_level=0, bits=bits)
        for full in (False, True):
            own = dict(raw_lut=lut(0))
            if full:
                own.update(raw_ccm=ccm(0), raw_curve=utils.raw_curve(1.0), raw_shading=shade(0))
            for k in [int(v) for v in a.ks.split(",") if v]:
                setups = [dict(raw_lut=lut(i + 1), **(dict(raw_ccm=ccm(i + 1), raw_shading=shade(i + 1)) if full else {})) for i in range(k)]
                groups = {"shared": LaneTrackerGroup(k, **cal, pixel_format=fmt, **own),
                          "distinct": LaneTrackerGroup(k, **cal, pixel_format=fmt, raw_setups=setups, **own)}
                cell = dict(bits=bits, stages="table + colour stage + shading map" if full else "table", k=k, ticks=a.ticks, rounds=a.rounds)
                try:
                    und = {m: [] for m in groups}
                    launches, tick = {}, {}
                    t = 0
                    for m, g in groups.items():
                        for _ in range(a.warmup):
                            g.process([frames[(t + 11 * i) % POOL] for i in range(k)])
                            t += 1
                    for r in range(a.rounds):
                        for m, g in groups.items():          # alternated: shared, distinct, shared, distinct, ...
                            ctx = g._ctx
                            ctx.sync()
                            ctx.set_stage_timing(True)
                            ctx.stage_reset()
                            for j in range(a.ticks):
                                g.process([frames[(r * a.ticks + j + 11 * i) % POOL] for i in range(k)])
                            ctx.sync()
                            ms = ctx.stage_ms()
                            ctx.set_stage_timing(False)
                            und[m].append(ms["undistort_rows"][0] / a.ticks)
                            launches[m] = round(ms["undistort_rows"][1] / a.ticks, 2)
                    for m, g in groups.items():
                        times = []
                        for j in range(a.ticks):
                            fr = [frames[(j + 11 * i) % POOL] for i in range(k)]
                            t0 = time.perf_counter()
                            g.process(fr)
                            times.append(time.perf_counter() - t0)
                        tick[m] = round(float(np.median(times)) * 1e3, 3)
                    for m, g in groups.items():
                        cell[m] = dict(raw_sets=g.raw_set_count(), raw_walk_form=g._ctx.last_raw_walk_form(), undistort_ms=round(float(np.median(und[m])), 4),
                                       undistort_ms_range=[round(min(und[m]), 4), round(max(und[m]), 4)], undistort_launches_per_tick=launches[m],
                                       tick_ms_median=tick[m])
                    cell["distinct_over_shared"] = round(cell["distinct"]["undistort_ms"] / cell["shared"]["undistort_ms"], 3)
                finally:
                    for g in groups.values():
                        g.close()
                print(json.dumps(cell), flush=True)
                cells.append(cell)
    doc = dict(tool="group_throughput --raw-sets", size="%dx%d" % (W, H), cells=cells)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--ks-1080p", default="1,8")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--no-solo", action="store_true", help="the group only (a kernel trace of the group's ticks)")
    ap.add_argument("--distinct-calibrations", action="store_true", help="every stream a camera of its own calibration")
    ap.add_argument("--front-end-times", action="store_true", help="a second pass with stage timers: undistortion and warp per tick")
    ap.add_argument("--frames-out", choices=("host", "sink", "inplace"), default="host", help="where the annotated frames of a tick go")
    ap.add_argument("--sink-format", choices=("rgb", "nv12", "i420"), default="nv12", help="the pixel format of --frames-out sink")
    ap.add_argument("--device-frames", action="store_true", help="the inputs are DeviceFrames (what --frames-out inplace needs)")
    ap.add_argument("--raw-sets", action="store_true", help="the raw-sets leg: one shared raw set against K distinct ones (see the docstring)")
    ap.add_argument("--rounds", type=int, default=3, help="--raw-sets: alternated rounds per cell")
    a = ap.parse_args()
    if a.raw_sets:
        return raw_sets_leg(a)
    if a.frames_out == "inplace" and not a.device_frames:
        ap.error("--frames-out inplace draws into the frames handed in: it needs --device-frames")
    plan = [("1280x720", calib.reference_calibration(), [int(v) for v in a.ks.split(",") if v]),
            ("1920x1080", calib.scaled_calibration(1.5), [int(v) for v in a.ks_1080p.split(",") if v])]
    out = open(a.out, "a") if a.out else None
    for size, cal, ks in plan:
        pool = pool_frames(cal)
        one_solo = None
        for k in ks:
            stages = dict(front_end=a.front_end_times)
            gw, gc, times = run_group(cal, pool, k, a.ticks, a.warmup, a.distinct_calibrations, stages, a.frames_out, a.sink_format, a.device_frames)
            stages.pop("front_end")
            n = k * a.ticks
            sw, sc = run_solo(cal, pool, k, a.ticks, a.warmup) if not a.no_solo else (float("nan"), float("nan"))
            solo_fps = n / sw
            if k == 1:
                one_solo = solo_fps
            line = dict(tool="group_throughput", size=size, k=k, ticks=a.ticks, group_fps=round(n / gw, 1),
                        tick_ms_median=round(float(np.median(times)) * 1e3, 3), tick_ms_p99=round(float(np.percentile(times, 99)) * 1e3, 3),
                        solo_fps=round(solo_fps, 1), group_cpu_s_per_frame=round(gc / n, 6), solo_cpu_s_per_frame=round(sc / n, 6),
                        vs_one_solo=None if one_solo is None else round(n / gw / one_solo, 2), **stages)
            s = json.dumps(line)
            print(s, flush=True)
            if out:
                out.write(s + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
