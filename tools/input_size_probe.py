#!/usr/bin/env python3
"""What frames of another size (`input_size=`, lt_set_input_size) cost, and that plain contexts did not move.

Legs (each in a fresh child process; the variants alternate, `--runs` runs each, default 3; device events and a synchronise around
every timed region -- lt_timer_start / lt_timer_stop):
  a   mask_run over 256 resident slots, 1280x720 frames, plain context          us per 256 frames     [parent tree and this tree]
  a2  row uploads (enqueued) + mask_run, 1280x720 frames, plain context         us per 256 frames     [parent tree and this tree]
  b   row uploads (enqueued; source rows into staging + k_resize_rows) + mask_run, 1920x1080 frames into a context with
      input_size=(1920, 1080)                                                   us per 256 frames     [this tree]
      b - a2 is what the feature adds per 256 frames (the larger copy over the bus and the resize); a against the parent's own
      spread shows that plain contexts did not move.
  c   process_stream(windows of 128 frames, annotate=False) frames/s: a 1080p input_size tracker [this tree] against a plain tracker
      fed the frames resized beforehand, from host memory [parent tree].
`--parent-tree DIR` is a checkout of the parent commit with its library built (its legs are skipped without it).  k_resize_rows' own
time comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/input_size_probe.py --leg b` run; its algorithmic bytes
are (358 * 1920 + 238 * 1280) * 3 per frame at the reference calibration.

  python tools/input_size_probe.py [--runs 3] [--parent-tree DIR] [--out profiles/input_size.json] [--commit HASH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SRC = 256, (1920, 1080)


def _frames(n, size, cal, round_trip=False):
    """n frames of `size`: a drifting synthetic lane at the calibration's size, resized on the host where `size` differs.  round_trip:
    what a 1080p camera's frames look like once a user has resized them to the calibration's size beforehand."""
    from lane_tracker_amd import synth, utils
    pool = synth.stream_lanes(16, seed=5, cal=cal)
    if tuple(size) != tuple(cal["img_size"]) or round_trip:
        pool = np.stack([utils.resize_linear(f, SRC) for f in pool])
    if round_trip:
        pool = np.stack([utils.resize_linear(f, cal["img_size"]) for f in pool])
    return np.ascontiguousarray(pool[np.arange(n) % len(pool)])


def leg(name):
    from lane_tracker_amd import _native, calib
    from lane_tracker_amd.lane_tracker import LaneTracker
    cal = calib.reference_calibration()
    if name == "c_sized" or name == "c_plain":
        sized = name == "c_sized"
        frames = _frames(128, SRC if sized else cal["img_size"], cal, round_trip=not sized)
        t = LaneTracker(**cal, input_size=SRC) if sized else LaneTracker(**cal)
        try:
            wins = [frames] * 7
            n, t0 = 0, None
            for k, out in enumerate(t.process_stream(wins, annotate=False)):
                if k == 0:
                    t0 = time.perf_counter()         # the first window warms buffers and code objects
                else:
                    n += len(out)
            return {"frames_per_s": n / (time.perf_counter() - t0)}
        finally:
            t.close()
    sized = name == "b"
    size = SRC if sized else cal["img_size"]
    frames = _frames(N, size, cal)
    ctx = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], capacity=N)
    try:
        if sized:
            ctx.set_input_size(SRC)
        fp = _native.filter_params()
        times = []
        for it in range(6):
            if name == "a":
                ctx.upload_frame_rows(frames)
                ctx.timer_start()
                ctx.mask_run(N, fp)
            else:
                ctx.timer_start()
                keep = ctx.upload_frame_rows(frames, enqueue=True)
                ctx.mask_run(N, fp)
            ms = ctx.timer_stop()
            if it:                       # the first pass warms
                times.append(ms * 1e3)
        return {"us_per_256": float(np.median(times)), "passes": times}
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    if a.leg:
        sys.path.insert(0, a.tree)
        print("LEG " + json.dumps(leg(a.leg)))
        return 0

    def child(tree, name):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--tree", tree], capture_output=True, text=True, timeout=600,
                           cwd=tree)
        line = [l for l in r.stdout.splitlines() if l.startswith("LEG ")]
        if r.returncode != 0 or not line:
            raise RuntimeError("leg %s in %s failed:\n%s" % (name, tree, (r.stdout + r.stderr)[-2000:]))
        return json.loads(line[-1][4:])
    plan = [("this", HERE, n) for n in ("a", "a2", "b", "c_sized")]
    if a.parent_tree:
        plan += [("parent", a.parent_tree, n) for n in ("a", "a2", "c_plain")]
    else:
        plan.append(("this", HERE, "c_plain"))
    res = {}
    for run in range(a.runs):            # the variants alternate: every run visits every leg of both trees
        for who, tree, name in sorted(plan, key=lambda p: (p[2], p[0])):
            res.setdefault("%s:%s" % (who, name), []).append(child(tree, name))
    out = {"commit": a.commit, "runs": a.runs, "frames": N, "input_size": list(SRC), "legs": {}}
    for key, runs in res.items():
        field = "frames_per_s" if "frames_per_s" in runs[0] else "us_per_256"
        v = [r[field] for r in runs]
        out["legs"][key] = {field: {"median": float(np.median(v)), "min": min(v), "max": max(v), "runs": v}}
    out["algorithmic_bytes_per_frame_resize"] = (358 * 1920 + 238 * 1280) * 3
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
