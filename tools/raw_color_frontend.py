#!/usr/bin/env python3
"""What the colour stage of raw Bayer input (lt_set_raw_color: colour-correction matrix + output curve behind the demosaic) costs.

    python tools/raw_color_frontend.py [--rounds 3] [--out profiles/raw_color_frontend.json]

Per round, for the 8-bit table form ('bayer_rggb' behind raw_lut(16, 240, (1.9, 1, 1.6))) and the 12-bit form ('bayer12_rggb' behind its
counterpart), on the slots' staging frames and on attached surfaces (dense pitch), WITHOUT and WITH the stage, back to back on one
context -- the kernels without the stage are the parent commit's walks, instruction for instruction (tests/test_raw_color_isa.py and
the three older ISA tests hold that) --:

    undistort_rows   the stage time of one mask run over 256 resident frames (lt_set_stage_timing), four streams: three warm runs, five
                     timed runs, every run listed
    stream           frames/s of a host-fed process_stream(annotate=False), windows of 128, sixty timed windows behind four warm ones, the
                     leg with the stage first (with few windows this leg measures the start-up, and whichever tracker comes second wins)

and the instruction counts' prediction beside them: VALU instructions per frame of the walk with and without the stage (DESIGN.md
section 4), whose ratio is what a walk bound by VALU issue should pay.  Prints one JSON document; writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lane_tracker_amd import _native, calib, synth, utils          # noqa: E402
from lane_tracker_amd.device import DeviceFrames                    # noqa: E402
from lane_tracker_amd.lane_tracker import LaneTracker               # noqa: E402

NL = 256
CAMERA = [[1.9, -0.7, -0.2], [-0.3, 1.6, -0.3], [0.0, -0.6, 1.6]]
# per-frame loop VALU of the walks (slots, surfaces): without the stage, with it
LOOP_VALU = {"bayer_rggb": ((177, 190), (249, 262)), "bayer12_rggb": ((197, 210), (281, 294))}


def mosaic(rgb):
    """RGGB: R at (even, even), G at (even, odd) and (odd, even), B at (odd, odd)."""
    out = np.empty(rgb.shape[:-1], np.uint8)
    out[..., 0::2, 0::2] = rgb[..., 0::2, 0::2, 0]
    out[..., 0::2, 1::2] = rgb[..., 0::2, 1::2, 1]
    out[..., 1::2, 0::2] = rgb[..., 1::2, 0::2, 1]
    out[..., 1::2, 1::2] = rgb[..., 1::2, 1::2, 2]
    return out


def frames_for(fmt, n):
    r = synth.SceneRenderer()
    pool = mosaic(np.stack([r.render(i)[0] for i in range(16)]))
    if fmt == "bayer12_rggb":
        pool = pool.astype(np.uint16) << 4
    return np.ascontiguousarray(pool[np.arange(n) % len(pool)])


def table_for(fmt):
    return utils.raw_lut(16, 240, (1.9, 1, 1.6)) if fmt == "bayer_rggb" else utils.raw_lut(256, 3840, (1.9, 1, 1.6), bits=12)


def summary(values):
    return dict(runs=[round(v, 1) for v in values], median=round(float(np.median(values)), 1), lo=round(min(values), 1), hi=round(max(values), 1))


def stage_us(cal, fmt, surfaces, stage, warm=3, timed=5):
    """-> [µs of undistort_rows per 256 frames] without the stage, and with it: one context, the stage switched between the two legs."""
    frames = frames_for(fmt, NL)
    ctx = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], capacity=NL)
    keep = None
    try:
        ctx.set_input_format(fmt)
        ctx.set_raw_lut(table_for(fmt))
        if surfaces:
            row = cal["img_size"][0] * (2 if fmt == "bayer12_rggb" else 1)
            keep = ctx.attach_device_frames(DeviceFrames.from_host(frames, fmt, pitch=row))
        else:
            ctx.upload_frames(frames)
        ctx.set_streams(4)
        fp = _native.filter_params()
        out = {}
        for name, on in (("without", False), ("with", True)):
            ctx.set_raw_color(*stage, enable=on)
            ctx.set_stage_timing(True)
            for _ in range(warm):
                ctx.mask_run(NL, fp)
            ctx.sync()
            runs = []
            for _ in range(timed):
                ctx.stage_reset()
                ctx.mask_run(NL, fp)
                ctx.sync()
                runs.append(1000.0 * float(ctx.stage_ms()["undistort_rows"][0]))
            ctx.set_stage_timing(False)
            out[name] = runs
        return out
    finally:
        ctx.close()
        del keep


def stream_rate(cal, fmt, stage, windows=60, warm=4, size=128):
    frames = frames_for(fmt, size)
    kw = dict(raw_ccm=stage[0], raw_curve=stage[1]) if stage else {}
    t = LaneTracker(**cal, pixel_format=fmt, raw_lut=table_for(fmt), **kw)
    try:
        n, t0 = 0, None
        for k, out in enumerate(t.process_stream([frames] * (windows + warm), annotate=False)):
            if k == warm - 1:           # the first windows pay the set-up
                t0 = time.perf_counter()
            elif k >= warm:
                n += len(out)
        return n / (time.perf_counter() - t0)
    finally:
        t.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cal = calib.reference_calibration()
    stage = (utils.raw_ccm(CAMERA), utils.raw_curve("srgb"))
    doc = dict(tool="tools/raw_color_frontend.py", frames=NL, stage="raw_ccm(%r), raw_curve('srgb')" % (CAMERA,), rounds=[], loop_valu=LOOP_VALU)
    for r in range(a.rounds):
        rnd = {}
        for fmt in ("bayer_rggb", "bayer12_rggb"):
            for surfaces in (False, True):
                got = stage_us(cal, fmt, surfaces, stage)
                rnd["%s/%s" % (fmt, "surfaces" if surfaces else "slots")] = {k: summary(v) for k, v in got.items()}
            with_stage = round(stream_rate(cal, fmt, stage), 1)
            rnd["%s/stream_fps" % fmt] = {"without": round(stream_rate(cal, fmt, None), 1), "with": with_stage}
        doc["rounds"].append(rnd)
        print(json.dumps({"round": r, **rnd}), flush=True)
    # medians of the rounds' medians, the range of all runs, the measured ratio beside the instruction counts'
    doc["summary"] = {}
    for key in doc["rounds"][0]:
        if key.endswith("stream_fps"):
            doc["summary"][key] = {w: summary([rd[key][w] for rd in doc["rounds"]]) for w in ("without", "with")}
            continue
        s = {}
        for w in ("without", "with"):
            allruns = [v for rd in doc["rounds"] for v in rd[key][w]["runs"]]
            s[w] = dict(median_of_medians=round(float(np.median([rd[key][w]["median"] for rd in doc["rounds"]])), 1), lo=min(allruns), hi=max(allruns))
        fmt, src = key.split("/")
        base, cc = LOOP_VALU[fmt]
        i = 1 if src == "surfaces" else 0
        s["measured_ratio"] = round(s["with"]["median_of_medians"] / s["without"]["median_of_medians"], 3)
        s["valu_ratio"] = round(cc[i] / base[i], 3)
        doc["summary"][key] = s
    text = json.dumps(doc, indent=1)
    print(json.dumps(doc["summary"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
