#!/usr/bin/env python3
"""What the lens-shading correction of raw Bayer input (lt_set_raw_shading: a gain per site from a mesh, in front of the raw table) costs.

    python tools/raw_shading_frontend.py [--rounds 3] [--out profiles/raw_shading_frontend.json]

Per round, for the 8-bit table form ('bayer_rggb' behind raw_lut(16, 240, (1.9, 1, 1.6))) and the 12-bit form ('bayer12_rggb' behind its
counterpart), each without and with the colour stage, on the slots' staging frames and on attached surfaces (dense pitch), WITHOUT and
WITH a map, back to back on one context -- the kernels without the map are the parent commit's walks, instruction for instruction
(tests/test_raw_shading_isa.py and the four older ISA tests hold that) --:

    undistort_rows   the stage time of one mask run over 256 resident frames (lt_set_stage_timing), four streams: three warm runs, five
                     timed runs, every run listed

and the instruction counts' prediction beside them: VALU instructions per frame of the walk with and without the map (DESIGN.md
section 4), whose ratio is what a walk bound by VALU issue should pay, and the VGPRs of the two.  The map is a camera-like 17 x 13
vignette, 1 + 1.5 r^2 times 1 / 1.05 / 1.05 / 1.1 per colour over the raw table's pedestal; what it holds does not change what runs.
Prints one JSON document; writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lane_tracker_amd import _native, calib, utils                  # noqa: E402
from lane_tracker_amd.device import DeviceFrames                    # noqa: E402
from raw_color_frontend import CAMERA, NL, frames_for, summary, table_for          # noqa: E402

# (format, colour stage) -> per-frame loop VALU of the walks (slots, surfaces) without the map and with it; the VGPRs likewise.  Copies of
# what tests/test_raw_shading_isa.py (FORMS, WRAPPED_VALU and its docstring's table) pins on the compiled code: when that test's numbers
# move, these move with them -- the test is the source, this table only sets the prediction beside the measurement.
LOOP_VALU = {("bayer_rggb", False): ((177, 190), (249, 262)), ("bayer_rggb", True): ((249, 262), (321, 334)),
             ("bayer12_rggb", False): ((197, 210), (277, 290)), ("bayer12_rggb", True): ((281, 294), (361, 374))}
VGPRS = {("bayer_rggb", False): ((49, 50), (76, 77)), ("bayer_rggb", True): ((50, 51), (76, 77)),
         ("bayer12_rggb", False): ((53, 54), (77, 78)), ("bayer12_rggb", True): ((54, 55), (78, 79))}


def vignette(fmt):
    bits = 12 if fmt == "bayer12_rggb" else 8
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    g = 1 + 1.5 * (x * x + y * y) / 2
    return utils.raw_shading(np.stack([g, 1.05 * g, 1.05 * g, 1.1 * g]), black_level=16 << (bits - 8), bits=bits)


def stage_us(cal, fmt, surfaces, color, warm=3, timed=5):
    """-> [µs of undistort_rows per 256 frames] without the map, and with it: one context, the map switched between the two legs."""
    frames = frames_for(fmt, NL)
    ctx = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], capacity=NL)
    keep = None
    try:
        ctx.set_input_format(fmt)
        ctx.set_raw_lut(table_for(fmt))
        if color:
            ctx.set_raw_color(utils.raw_ccm(CAMERA), utils.raw_curve("srgb"))
        if surfaces:
            row = cal["img_size"][0] * (2 if fmt == "bayer12_rggb" else 1)
            keep = ctx.attach_device_frames(DeviceFrames.from_host(frames, fmt, pitch=row))
        else:
            ctx.upload_frames(frames)
        ctx.set_streams(4)
        fp = _native.filter_params()
        out = {}
        for name, on in (("without", False), ("with", True)):
            ctx.set_raw_shading(vignette(fmt) if on else None)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cal = calib.reference_calibration()
    forms = [(fmt, color) for fmt in ("bayer_rggb", "bayer12_rggb") for color in (False, True)]
    key_of = lambda fmt, color, surfaces: "%s%s/%s" % (fmt, "+color" if color else "", "surfaces" if surfaces else "slots")
    doc = dict(tool="tools/raw_shading_frontend.py", frames=NL, map="17 x 13 vignette, 1 + 1.5 r^2, x 1 / 1.05 / 1.05 / 1.1, black 16 / 256",
               rounds=[], loop_valu={key_of(f, c, False).split("/")[0]: v for (f, c), v in LOOP_VALU.items()},
               vgprs={key_of(f, c, False).split("/")[0]: v for (f, c), v in VGPRS.items()})
    for r in range(a.rounds):
        rnd = {}
        for fmt, color in forms:
            for surfaces in (False, True):
                got = stage_us(cal, fmt, surfaces, color)
                rnd[key_of(fmt, color, surfaces)] = {k: summary(v) for k, v in got.items()}
        doc["rounds"].append(rnd)
        print(json.dumps({"round": r, **rnd}), flush=True)
    # medians of the rounds' medians, the range of all runs, the measured ratio beside the instruction counts'
    doc["summary"] = {}
    for fmt, color in forms:
        for surfaces in (False, True):
            key, s = key_of(fmt, color, surfaces), {}
            for w in ("without", "with"):
                allruns = [v for rd in doc["rounds"] for v in rd[key][w]["runs"]]
                s[w] = dict(median_of_medians=round(float(np.median([rd[key][w]["median"] for rd in doc["rounds"]])), 1), lo=min(allruns), hi=max(allruns))
            base, ls = LOOP_VALU[(fmt, color)]
            i = 1 if surfaces else 0
            s["measured_ratio"] = round(s["with"]["median_of_medians"] / s["without"]["median_of_medians"], 3)
            s["valu_ratio"] = round(ls[i] / base[i], 3)
            doc["summary"][key] = s
    text = json.dumps(doc, indent=1)
    print(json.dumps(doc["summary"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
