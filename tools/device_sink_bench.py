#!/usr/bin/env python3
"""What the device sinks cost and buy: the store kernels alone (k_sink.hip) against the copy ceiling, and process_stream with
annotated frames leaving through a sink beside the host-out forms of the same stream.

Modes (both by default; every leg runs `--runs` times, the legs of a mode taking turns run by run; the file holds each run, the
median and the range, and the commit):
  --kernels   lt_rgb_to_surfaces over 256 dense RGB frames of 1280x720 into RGB, NV12 and I420 sinks: the wide form (dense sinks,
              16-byte aligned) and the byte-wise form (the same sinks one byte further on).  A call is synchronous -- 8 launches of
              32 surfaces and one wait -- so the host clock around it is launch overhead + kernel time; us per 256 frames, the
              bytes the conversion has to move, and their share of the copy ceiling DESIGN.md section 5.2 uses (6.29 TB/s).
  --stream    process_stream, windows of 128 frames with a short outage, at 1280x720 and 1920x1080, frames/s behind the first
              window: DeviceFrames in and sink out (RGB -> RGB, NV12 -> NV12); host arrays in and annotated frames out through
              the host (annotate=True: the copy threads place them); annotate='inplace'; and search only (annotate=False,
              DeviceFrames in) -- the stream whose spread the device-out form should share; and DeviceFrames in, drawn into in
              place (out="inplace": RGB, NV12, I420) -- every window a fresh copy of the frames, made ahead of the clock.

  python tools/device_sink_bench.py [--kernels | --stream] [--runs 3] [--out profiles/device_sink.json] [--commit HASH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lane_tracker_amd import _native, calib, synth  # noqa: E402
from lane_tracker_amd.device import DeviceBuffer, DeviceFrames  # noqa: E402
from lane_tracker_amd.lane_tracker import LaneTracker  # noqa: E402

COPY_CEILING_TBS = 6.29
POOL, NL = 32, 256


def summary(values, digits=1):
    return dict(runs=[round(v, digits) for v in values], median=round(float(np.median(values)), digits), lo=round(min(values), digits),
                hi=round(max(values), digits))


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


# ---- the store kernels -----------------------------------------------------------------------------------------------------------
def kernel_legs(runs, reps, note):
    w, h = calib.IMAGE_WIDTH_HEIGHT
    frame = w * h * 3
    rgb = np.random.default_rng(3).integers(0, 256, (POOL, h, w, 3), dtype=np.uint8)
    with DeviceBuffer(NL * frame) as src:
        for k in range(NL // POOL):
            src.copy_from_host(rgb, offset=k * POOL * frame)
        legs = [(layout, form) for layout in ("rgb", "nv12", "i420") for form in ("wide", "bytewise")]
        sinks = {(layout, form): DeviceFrames.empty(NL, (w, h), layout, offset=0 if form == "wide" else 1) for layout, form in legs}
        times = {leg: [] for leg in legs}
        try:
            for leg in legs:             # every shape once ahead of the clock (code objects, the cache's blocks)
                _native.rgb_to_surfaces(src.ptr, frame, (w, h), sinks[leg])
            for _ in range(runs):
                for leg in legs:
                    best = []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        _native.rgb_to_surfaces(src.ptr, frame, (w, h), sinks[leg])
                        best.append((time.perf_counter() - t0) * 1e6)
                    times[leg].append(float(np.median(best)))
        finally:
            for s in sinks.values():
                s.owner.close()
    for layout, form in legs:
        moved = NL * (frame + (frame if layout == "rgb" else frame // 2))
        s = summary(times[(layout, form)])
        note(dict(leg="store_kernels", layout=layout, form=form, frames=NL, size="%dx%d" % (w, h), launches=NL // 32, reps_per_run=reps, us_per_256_frames=s,
                  bytes_moved=moved, TBs_at_median=round(moved / (s["median"] * 1e-6) / 1e12, 3),
                  share_of_copy_ceiling=round(moved / (s["median"] * 1e-6) / 1e12 / COPY_CEILING_TBS, 3)))


# ---- the stream --------------------------------------------------------------------------------------------------------------------
_pools = {}


def frames_for(cal, fmt):
    key = (tuple(cal["img_size"]), fmt)
    if key not in _pools:
        pool = synth.stream_lanes(POOL, seed=5, cal=cal).copy()
        pool[20:23] = 0                  # a short outage: second tries, failure pictures
        if fmt != "rgb":
            pool = np.stack([rgb_to_nv12(f) for f in pool])
            if fmt == "i420":            # the same samples, U and V in planes of their own
                h = pool.shape[1] * 2 // 3
                uv = pool[:, h:].reshape(len(pool), -1, 2)
                pool = np.concatenate([pool[:, :h].reshape(len(pool), -1), uv[..., 0], uv[..., 1]], 1).reshape(pool.shape)
        _pools[key] = pool
    return np.ascontiguousarray(_pools[key][np.arange(128) % POOL])


def leg_stream(cal, form, windows=6, size=128):
    """frames/s of `windows` windows behind the first one (which pays the set-up)."""
    fmt = "nv12" if "nv12" in form else ("i420" if "i420" in form else "rgb")
    frames = frames_for(cal, fmt)
    t = LaneTracker(**cal) if fmt == "rgb" else LaneTracker(**cal, pixel_format=fmt)
    keep = []
    try:
        kw = dict(annotate=True)
        win = frames
        if form.startswith("device_"):
            win = DeviceFrames.from_host(frames, fmt)
            keep.append(win)
            if form == "device_search_only":
                kw = dict(annotate=False)
            elif form.endswith("_inplace"):
                kw = dict(out="inplace")
            else:
                sinks = [DeviceFrames.empty(size, cal["img_size"], fmt) for _ in range(4)]     # one being filled, one landing, one with the caller, one to spare
                keep += sinks
                kw = dict(out=(sinks[k % 4] for k in range(windows + 1)))
        elif form == "host_inplace":
            kw = dict(annotate="inplace")
        feed = ([win.copy() for _ in range(windows + 1)] if form == "host_inplace" else [win] * (windows + 1))
        if form.startswith("device_") and form.endswith("_inplace"):     # a drawn window is no camera window any more: fresh ones
            feed = [win] + [DeviceFrames.from_host(frames, fmt) for _ in range(windows)]
            keep += feed[1:]
        n, t0 = 0, None
        for k, out in enumerate(t.process_stream(feed, **kw)):
            if k == 0:
                t0 = time.perf_counter()
            else:
                n += len(out)
        return n / (time.perf_counter() - t0)
    finally:
        t.close()
        for f in keep:
            f.owner.close()


def stream_legs(runs, sizes, note):
    cals = {"1280x720": calib.reference_calibration, "1920x1080": lambda: calib.scaled_calibration(1.5)}
    forms = ("device_rgb_to_rgb_sink", "device_nv12_to_nv12_sink", "device_rgb_inplace", "device_nv12_inplace", "device_i420_inplace",
             "host_annotated", "host_inplace", "device_search_only")
    for size in sizes:
        cal = cals[size]()
        got = {f: [] for f in forms}
        for _ in range(runs):
            for f in forms:
                got[f].append(leg_stream(cal, f))
        for f in forms:
            s = summary(got[f])
            note(dict(leg="process_stream", size=size, form=f, frames_per_s=s, spread=round(s["hi"] / s["lo"], 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="calls per run of a store-kernel leg (the run's figure is their median)")
    ap.add_argument("--sizes", default="1280x720,1920x1080")
    ap.add_argument("--out", default="-")
    ap.add_argument("--commit", default=None, help="the commit hash to record (default: git rev-parse HEAD of this checkout)")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = None
    result = dict(tool="device_sink_bench", commit=commit, runs=a.runs, copy_ceiling_TBs=COPY_CEILING_TBS, legs=[])

    def note(line):
        result["legs"].append(line)
        print(json.dumps(line), flush=True)
    both = not (a.kernels or a.stream)
    if a.kernels or both:
        kernel_legs(a.runs, a.reps, note)
    if a.stream or both:
        stream_legs(a.runs, a.sizes.split(","), note)
    if a.out and a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
