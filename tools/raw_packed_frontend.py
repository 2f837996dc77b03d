#!/usr/bin/env python3
"""What MIPI-packed RAW10 / RAW12 input ('bayer10p_*' / 'bayer12p_*': unpacked in the walk) costs and saves against the same samples in
16-bit words ('bayer10_*' / 'bayer12_*').

    python tools/raw_packed_frontend.py [--rounds 2] [--out profiles/raw_packed_frontend.json]

Per round, for 10 and 12 bits, on the slots' staging frames and on attached surfaces (dense pitch), for the four stage combinations (the
table alone, + colour stage, + shading map, + both), the packed and the 16-bit context side by side, their timed runs ALTERNATING -- the
16-bit kernels are the parent commit's, instruction for instruction (tests/test_raw_packed_isa.py and the older ISA tests hold that) --:

    undistort_rows   the stage time of one mask run over 256 resident frames of 1280 x 720 (lt_set_stage_timing), four streams: three warm
                     runs, five timed runs each, every run listed

with the instruction counts' prediction beside it: the VALU instructions per frame of the two walks, whose ratio is what
a walk bound by VALU issue should pay, and their VGPRs; and

    process_stream   frames/s of a host-fed stream (windows of 128 frames, annotate=False), packed against 16-bit, alternating: the packed
                     frames are 0.625 (RAW10) and 0.75 (RAW12) of the words' bytes over the bus

Prints one JSON document; writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lane_tracker_amd import _native, calib, utils                  # noqa: E402
from lane_tracker_amd.device import DeviceFrames                    # noqa: E402
from lane_tracker_amd.lane_tracker import LaneTracker               # noqa: E402
from raw_color_frontend import CAMERA, NL, frames_for, summary      # noqa: E402

COMBOS = (("table", False, False), ("+color", True, False), ("+shading", False, True), ("+both", True, True))
# (bits, combination) -> per-frame loop VALU of the walks (slots, surfaces), 16-bit and packed; the VGPRs likewise.  Copies of what
# tests/test_raw_packed_isa.py (FORMS, and test_raw_lut_isa.STAGES_LOOP_VALU) pins on the compiled code: the test is the source, this table
# only sets the prediction beside the measurement.
WORDS_VALU = {"table": (197, 210), "+color": (281, 294), "+shading": (277, 290), "+both": (361, 374)}
WORDS_VGPRS = {"table": (53, 54), "+color": (54, 55), "+shading": (77, 78), "+both": (78, 79)}
PACKED_VGPRS = {(10, "table"): (67, 69), (10, "+color"): (68, 69), (10, "+shading"): (87, 93), (10, "+both"): (93, 94),
                (12, "table"): (66, 68), (12, "+color"): (67, 69), (12, "+shading"): (85, 92), (12, "+both"): (92, 93)}
ADDS = {10: 56, 12: 48}


def packed_valu(bits, combo):
    return tuple(v + ADDS[bits] for v in WORDS_VALU[combo])


def words_for(bits, n):
    """n frames of the scene pool as `bits`-bit samples in 16-bit words."""
    return np.ascontiguousarray(frames_for("bayer12_rggb", n) >> (12 - bits))


def table_for(bits):
    return utils.raw_lut(256 >> (12 - bits), 3840 >> (12 - bits), (1.9, 1, 1.6), bits=bits)


def vignette(bits):
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    g = 1 + 1.5 * (x * x + y * y) / 2
    return utils.raw_shading(np.stack([g, 1.05 * g, 1.05 * g, 1.1 * g]), black_level=16 << (bits - 8), bits=bits)


def stage_us(cal, bits, surfaces, warm=3, timed=5):
    """-> {combination: {'words': [µs of undistort_rows per 256 frames], 'packed': [...]}}: two contexts, their timed runs alternating."""
    fmts = {"words": "bayer%d_rggb" % bits, "packed": "bayer%dp_rggb" % bits}
    words = words_for(bits, NL)
    frames = {"words": words, "packed": utils.pack_raw(words, fmts["packed"])}
    ctxs, keep = {}, []
    try:
        for k, fmt in fmts.items():
            c = ctxs[k] = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], capacity=NL)
            c.set_input_format(fmt)
            c.set_raw_lut(table_for(bits))
            if surfaces:
                keep.append(c.attach_device_frames(DeviceFrames.from_host(frames[k], fmt, pitch=frames[k].shape[-1] * frames[k].itemsize)))
            else:
                c.upload_frames(frames[k])
            c.set_streams(4)
        fp = _native.filter_params()
        out = {}
        for combo, cc, ls in COMBOS:
            for c in ctxs.values():
                c.set_raw_color(utils.raw_ccm(CAMERA) if cc else None, utils.raw_curve("srgb") if cc else None, enable=cc)
                c.set_raw_shading(vignette(bits) if ls else None)
                c.set_stage_timing(True)
                for _ in range(warm):
                    c.mask_run(NL, fp)
                c.sync()
            runs = {k: [] for k in ctxs}
            for _ in range(timed):
                for k, c in ctxs.items():
                    c.stage_reset()
                    c.mask_run(NL, fp)
                    c.sync()
                    runs[k].append(1000.0 * float(c.stage_ms()["undistort_rows"][0]))
            for c in ctxs.values():
                c.set_stage_timing(False)
            out[combo] = runs
        return out
    finally:
        for c in ctxs.values():
            c.close()
        for d in keep:
            d.owner.close()


def stream_rates(cal, bits, windows=24, warm=3, size=128, legs=2):
    """-> {'words': [frames/s per leg], 'packed': [...]}: host-fed process_stream without annotation, the two formats' legs alternating."""
    words = words_for(bits, size)
    fmts = {"words": ("bayer%d_rggb" % bits, words), "packed": ("bayer%dp_rggb" % bits, utils.pack_raw(words, "bayer%dp_rggb" % bits))}
    out = {k: [] for k in fmts}
    for _ in range(legs):
        for k, (fmt, frames) in fmts.items():
            t = LaneTracker(**cal, pixel_format=fmt, raw_lut=table_for(bits))
            try:
                n, t0 = 0, None
                for i, res in enumerate(t.process_stream([frames] * (windows + warm), annotate=False)):
                    if i == warm - 1:       # the first windows pay the set-up
                        t0 = time.perf_counter()
                    elif i >= warm:
                        n += len(res)
                out[k].append(round(n / (time.perf_counter() - t0), 1))
            finally:
                t.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cal = calib.reference_calibration()
    key_of = lambda bits, combo, surfaces: "raw%d %s/%s" % (bits, combo, "surfaces" if surfaces else "slots")
    doc = dict(tool="tools/raw_packed_frontend.py", frames=NL, image="%dx%d" % tuple(cal["img_size"]), bus_bytes_ratio={"raw10": 0.625, "raw12": 0.75}, rounds=[],
               loop_valu={"raw%d %s" % (b, c): dict(words=WORDS_VALU[c], packed=packed_valu(b, c)) for b in (10, 12) for c, _, _ in COMBOS},
               vgprs={"raw%d %s" % (b, c): dict(words=WORDS_VGPRS[c], packed=PACKED_VGPRS[b, c]) for b in (10, 12) for c, _, _ in COMBOS})
    for r in range(a.rounds):
        rnd = {}
        for bits in (10, 12):
            for surfaces in (False, True):
                for combo, runs in stage_us(cal, bits, surfaces).items():
                    rnd[key_of(bits, combo, surfaces)] = {k: summary(v) for k, v in runs.items()}
            rnd["raw%d process_stream fps" % bits] = stream_rates(cal, bits)
        doc["rounds"].append(rnd)
        print(json.dumps({"round": r, **rnd}), flush=True)
    # medians of the rounds' medians, the range of all runs, the measured ratio beside the instruction counts'
    doc["summary"] = {}
    for bits in (10, 12):
        for combo, _, _ in COMBOS:
            for surfaces in (False, True):
                key, s = key_of(bits, combo, surfaces), {}
                for w in ("words", "packed"):
                    allruns = [v for rd in doc["rounds"] for v in rd[key][w]["runs"]]
                    s[w] = dict(median_of_medians=round(float(np.median([rd[key][w]["median"] for rd in doc["rounds"]])), 1), lo=min(allruns), hi=max(allruns))
                i = 1 if surfaces else 0
                s["measured_ratio"] = round(s["packed"]["median_of_medians"] / s["words"]["median_of_medians"], 3)
                s["valu_ratio"] = round(packed_valu(bits, combo)[i] / WORDS_VALU[combo][i], 3)
                doc["summary"][key] = s
        fps = {w: [v for rd in doc["rounds"] for v in rd["raw%d process_stream fps" % bits][w]] for w in ("words", "packed")}
        doc["summary"]["raw%d process_stream fps" % bits] = dict(words=summary(fps["words"]), packed=summary(fps["packed"]),
                                                                ratio=round(float(np.median(fps["packed"]) / np.median(fps["words"])), 3))
    text = json.dumps(doc, indent=1)
    print(json.dumps(doc["summary"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
