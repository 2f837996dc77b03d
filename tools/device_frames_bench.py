#!/usr/bin/env python3
"""What frames that are already in device memory cost and buy: the batch step over attached surfaces beside the same step over
slot-resident frames, and the tracker's entry points fed from the device beside the same calls fed from the host.

Modes (one per invocation; every leg runs `--runs` times, the file holds each run, the median and the range, and the commit):
  --resident   the batch step of bench.py -- 256 frames, mask chain + sliding-window search + fit, `--steps` steps behind
               `--warmup` -- over frames that lie in the context's own slots (lt_upload_frames once), RGB and NV12.  Uses only
               calls an older checkout has too, so the same file run from such a checkout gives the yardstick.
  --attached   the same step over frames attached where they lie (lt_attach_device_frames): RGB dense, NV12 dense, NV12 at a
               pitch of W + 64.
  --trackers   process_stream (plain, windows of 128) at 1280x720 and 1920x1080, RGB and NV12; process() annotated; a
               LaneTrackerGroup of 8 -- each fed DeviceFrames and, beside it, host arrays.
  --host-fed   the host-fed halves of --trackers alone (what an older checkout can run: its figures are the yardstick).

`--pixel-format yuy2|uyvy|bgr|rgba|bgra|bayer_rggb|bayer_grbg|bayer_gbrg|bayer_bggr` (repeatable) adds packed 4:2:2 legs, legs in the RGB
family's other members, or 8-bit raw Bayer legs to `--formats`; `--legs stream` keeps the process_stream leg alone of --trackers / --host-fed; with --resident / --attached every leg also records
the `undistort_rows` stage time per 256 frames (lt_set_stage_timing: one timed mask run behind the measured steps).

The `--runs` repetitions of a leg run back to back, one format after the other.  For runs that ALTERNATE between the formats (what
profiles/yuv422_frontend.json holds) call the tool once per round with `--runs 1` and a file of its own, and put the rounds together.

  python tools/device_frames_bench.py --attached [--runs 3] [--steps 10] [--warmup 2] [--out profiles/device_frames.json] [--commit HASH]
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
from lane_tracker_amd.lane_tracker import LaneTracker  # noqa: E402

try:
    from lane_tracker_amd.device import DeviceFrames  # noqa: E402
except ImportError:                     # a checkout without device-resident input: --resident and --host-fed still run
    DeviceFrames = None
HAS_YUV = hasattr(_native.Context, "set_input_format")
POOL, NL = 32, 256


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


def rgb_to_422(rgb, fmt):
    """BT.601 video range, chroma the mean of each pixel pair; 'yuy2': Y0 U Y1 V, 'uyvy': U Y0 V Y1 (only makes inputs)."""
    f = rgb.astype(np.float32)
    h, w = f.shape[:2]
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    y = q(0.257 * r + 0.504 * g + 0.098 * b + 16)
    u = q((-0.148 * r - 0.291 * g + 0.439 * b + 128).reshape(h, w // 2, 2).mean(2))
    v = q((0.439 * r - 0.368 * g - 0.071 * b + 128).reshape(h, w // 2, 2).mean(2))
    m = np.stack([y[:, 0::2], u, y[:, 1::2], v] if fmt == "yuy2" else [u, y[:, 0::2], v, y[:, 1::2]], -1)
    return m.reshape(h, w, 2)


PACKED = ("yuy2", "uyvy")
RGB_FAMILY = ("bgr", "rgba", "bgra")
BAYER = ("bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr")
ROW_BYTES = dict(rgb=3, yuy2=2, uyvy=2, bgr=3, rgba=4, bgra=4)          # bytes a pixel of plane 0 (1: the 4:2:0 formats and raw Bayer)


def rgb_to_bayer(rgb, fmt):
    """The mosaic of RGB frames (n, H, W, 3): every site keeps the channel the pattern's name gives it (only makes inputs)."""
    ch = ["rgb".index(c) for c in fmt[len("bayer_"):]]
    out = np.empty(rgb.shape[:-1], np.uint8)
    for i, c in enumerate(ch):
        out[:, i >> 1::2, i & 1::2] = rgb[:, i >> 1::2, i & 1::2, c]
    return out


def rgb_to_family(rgb, fmt):
    from lane_tracker_amd.utils import rgb_to_packed
    return rgb_to_packed(rgb, fmt, alpha=0x5a)
_pools = {}


def frames_for(cal, fmt, n, outage=False):
    key = (tuple(cal["img_size"]), fmt, outage)
    if key not in _pools:
        pool = synth.stream_lanes(POOL, seed=5, cal=cal).copy()
        if outage:
            pool[20:23] = 0             # a short outage: second tries, failure pictures
        _pools[key] = (np.stack([rgb_to_nv12(f) for f in pool]) if fmt == "nv12" else
                       np.stack([rgb_to_422(f, fmt) for f in pool]) if fmt in PACKED else
                       rgb_to_family(pool, fmt) if fmt in RGB_FAMILY else rgb_to_bayer(pool, fmt) if fmt in BAYER else pool)
    return np.ascontiguousarray(_pools[key][np.arange(n) % POOL])


def summary(values):
    return dict(runs=[round(v, 1) for v in values], median=round(float(np.median(values)), 1), lo=round(min(values), 1), hi=round(max(values), 1))


# ---- the batch step ------------------------------------------------------------------------------------------------------------
def batch_step(cal, fmt, mode, steps, warmup, streams, pitch_extra=0):
    """frames/s of `steps` steps (mask chain + sliding-window search + fit over 256 frames) behind `warmup`; lanes detected; ms of
    the undistort_rows stage of one more mask run over the 256 frames, timed stage by stage (None where the library cannot)."""
    frames = frames_for(cal, fmt, NL)
    ctx = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], capacity=2 * NL)
    keep = None
    try:
        if fmt != "rgb":
            ctx.set_input_format(fmt)
        if mode == "resident":
            ctx.upload_frames(frames)
        else:
            row = cal["img_size"][0] * ROW_BYTES.get(fmt, 1)
            keep = ctx.attach_device_frames(DeviceFrames.from_host(frames, fmt, pitch=row + pitch_extra))
        fp, sp = _native.filter_params(), _native.search_params()
        ctx.set_streams(streams)

        def step():
            ctx.mask_run(NL, fp)
            ctx.sws_fit_run(NL, sp)
        for _ in range(warmup):
            step()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        ctx.sync()
        dt = time.perf_counter() - t0
        rec = ctx.download_records(NL)
        stage = None
        if hasattr(ctx, "set_stage_timing"):
            ctx.set_stage_timing(True)
            ctx.mask_run(NL, fp)            # (the first timed run pays for the events)
            ctx.sync()
            ctx.stage_reset()
            ctx.mask_run(NL, fp)
            ctx.sync()
            stage = float(ctx.stage_ms()["undistort_rows"][0])
            ctx.set_stage_timing(False)
        return NL * steps / dt, int((rec["detected"] != 0).sum()), stage
    finally:
        ctx.close()
        del keep


# ---- the tracker's entry points --------------------------------------------------------------------------------------------------
def tracker(cal, fmt):
    return LaneTracker(**cal) if fmt == "rgb" else LaneTracker(**cal, pixel_format=fmt)


def leg_stream(cal, fmt, frames, device, windows=6, size=128):
    t = tracker(cal, fmt)
    try:
        win = DeviceFrames.from_host(frames[:size], fmt) if device else frames[:size]
        n, t0 = 0, None
        for k, out in enumerate(t.process_stream([win] * (windows + 1), annotate=False)):
            if k == 0:                  # the first window pays the set-up
                t0 = time.perf_counter()
            else:
                n += len(out)
        return n / (time.perf_counter() - t0)
    finally:
        t.close()


def leg_process(cal, fmt, frames, device, n=150, warm=20):
    t = tracker(cal, fmt)
    try:
        src = DeviceFrames.from_host(frames[:POOL], fmt) if device else frames
        for k in range(warm):
            t.process(src[k % POOL])
        t0 = time.perf_counter()
        for k in range(n):
            t.process(src[(warm + k) % POOL])
        return n / (time.perf_counter() - t0)
    finally:
        t.close()


def leg_group(cal, fmt, frames, device, k=8, ticks=60, warm=10, annotate=True):
    from lane_tracker_amd.group import LaneTrackerGroup
    kw = {} if fmt == "rgb" else dict(pixel_format=fmt)
    g = LaneTrackerGroup(k, **cal, **kw)
    try:
        src = DeviceFrames.from_host(frames[:POOL], fmt) if device else frames
        tick = lambda j: [src[(j + 3 * i) % POOL] for i in range(k)]
        for j in range(warm):
            g.process(tick(j), annotate=annotate)
        t0 = time.perf_counter()
        for j in range(ticks):
            g.process(tick(warm + j), annotate=annotate)
        return k * ticks / (time.perf_counter() - t0)
    finally:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    m = ap.add_mutually_exclusive_group(required=True)
    m.add_argument("--resident", action="store_true")
    m.add_argument("--attached", action="store_true")
    m.add_argument("--trackers", action="store_true")
    m.add_argument("--host-fed", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--sizes", default="1280x720,1920x1080")
    ap.add_argument("--formats", default="rgb,nv12")
    ap.add_argument("--pixel-format", action="append", choices=PACKED + RGB_FAMILY + BAYER, default=[],
                    help="a packed 4:2:2 format, another member of the RGB family, or an 8-bit raw Bayer pattern, to measure beside --formats (repeatable)")
    ap.add_argument("--legs", choices=("all", "stream"), default="all", help="--trackers / --host-fed: every leg, or process_stream alone")
    ap.add_argument("--out", default="-")
    ap.add_argument("--commit", default=None, help="the commit hash to record (default: git rev-parse HEAD of this checkout)")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = None
    mode = "resident" if a.resident else "attached" if a.attached else "trackers" if a.trackers else "host_fed"
    if mode in ("attached", "trackers") and DeviceFrames is None:
        sys.exit("this checkout has no device-resident input: only --resident and --host-fed run here")
    result = dict(tool="device_frames_bench", mode=mode, commit=commit, runs=a.runs, legs=[])

    def note(line):
        result["legs"].append(line)
        print(json.dumps(line), flush=True)
    formats = [f for f in a.formats.split(",") + a.pixel_format if f == "rgb" or HAS_YUV]
    if any(f in PACKED for f in formats) and "yuy2" not in getattr(_native, "INPUT_FORMATS", {}):
        sys.exit("this checkout has no packed 4:2:2 input")
    if any(f in RGB_FAMILY for f in formats) and "bgr" not in getattr(_native, "RGB_FAMILY", {}):
        sys.exit("this checkout has no BGR / RGBA / BGRA input")
    if any(f in BAYER for f in formats) and not hasattr(_native, "BAYER_FORMATS"):
        sys.exit("this checkout has no raw Bayer input")
    if mode in ("resident", "attached"):
        cal = calib.reference_calibration()
        for fmt in formats:
            for extra in ([0] if (mode == "resident" or fmt == "rgb") else [0, 64]):
                got = [batch_step(cal, fmt, mode, a.steps, a.warmup, a.streams, extra) for _ in range(a.runs)]
                line = dict(leg="batch_step", frames=mode, pixel_format=fmt, pitch_extra=extra, steps=a.steps, detected=got[0][1],
                            **summary([g[0] for g in got]))
                if got[0][2] is not None:
                    line["undistort_rows_ms_per_256"] = [round(g[2], 4) for g in got]
                note(line)
    else:
        cals = {"1280x720": calib.reference_calibration, "1920x1080": lambda: calib.scaled_calibration(1.5)}
        feeds = [False] if mode == "host_fed" else [True, False]
        for size in a.sizes.split(","):
            cal = cals[size]()
            for fmt in formats:
                frames = frames_for(cal, fmt, NL, outage=True)
                for device in feeds:
                    note(dict(leg="process_stream", size=size, pixel_format=fmt, fed="device" if device else "host",
                              **summary([leg_stream(cal, fmt, frames, device) for _ in range(a.runs)])))
                if size != "1280x720" or a.legs == "stream":
                    continue
                for device in feeds:
                    note(dict(leg="process_annotated", size=size, pixel_format=fmt, fed="device" if device else "host",
                              **summary([leg_process(cal, fmt, frames, device) for _ in range(a.runs)])))
                    if hasattr(LaneTracker, "process") and os.path.exists(os.path.join(ROOT, "lane_tracker_amd", "group.py")):
                        note(dict(leg="group_k8_annotated", size=size, pixel_format=fmt, fed="device" if device else "host",
                                  **summary([leg_group(cal, fmt, frames, device) for _ in range(a.runs)])))
    if a.out and a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
