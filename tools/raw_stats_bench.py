"""Times lt_raw_stats (k_raw_stats.hip) on the device: N slots of the reference calibration's 1280 x 720 at the default rectangle, for 8-bit
bytes, 12-bit words and RAW12, each on a random frame and on an all-equal one (every site of a phase in one bin: what same-bin contention
costs), beside the undistort_rows stage time of the same format and batch in the same sitting.

    python tools/raw_stats_bench.py [--slots 256] [--reps 20] [--out profiles/raw_stats.json]

Per case: call_ms, the whole call with all three outputs (a wait for the context, the scratch's memset, the kernel, the copies to the host, the
host's wait); nocopy_ms, the same call with no output asked for (no copies) -- still the HOST's clock around the wait for the context, the
memset, the launch and the wait for the stream, not a device time: an upper bound of the kernel's; bytes = the rectangle's bytes of the N
frames, read once by the definition (the 12-bit kernels read the cells' bottom rows twice); gbps = bytes / nocopy_ms, a lower bound of the
kernel's rate.  Medians of `reps` calls after two warm-up calls.  Every result is checked against utils.raw_stats on one slot first."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lane_tracker_amd import _native, calib, utils  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    n = a.slots
    out = {"slots": n, "img_size": [W, H], "reps": a.reps, "cases": []}
    for fmt in ("bayer_rggb", "bayer12_rggb", "bayer12p_rggb"):
        bits = _native.raw_bits(fmt)
        ctx = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], capacity=n)
        try:
            ctx.set_input_format(fmt)
            rows = _native.default_stats_rows(ctx.input_rows())
            tail = _native.frame_shape((W, H), fmt)
            row_bytes = tail[1] * _native.frame_dtype(fmt).itemsize
            nbytes = n * (rows[1] - rows[0]) * row_bytes
            rng = np.random.default_rng(bits)
            for content in ("random", "all equal"):
                if content == "random":
                    one = rng.integers(0, 256 if _native.frame_dtype(fmt).itemsize == 1 else 1 << bits, tail).astype(_native.frame_dtype(fmt))
                else:
                    flat = np.full((H, W), (1 << bits) // 3, np.uint16)
                    one = flat.astype(np.uint8) if bits == 8 else utils.pack_raw(flat, fmt) if fmt in _native.BAYER_PACKED_FORMATS else flat
                frames = np.ascontiguousarray(np.broadcast_to(one, (16,) + tail))
                for at in range(0, n, 16):
                    ctx.upload_frames(frames[:min(16, n - at)], first=at)
                got, want = ctx.raw_stats(1, n - 1), utils.raw_stats(one[None], fmt, rows=rows)
                assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])), (fmt, content)
                p = _native.checked_raw_stats(fmt, (W, H), ctx.input_rows())

                def without_copies():
                    _native._check(ctx.lib.lt_raw_stats(ctx._h, 0, n, C.byref(p), None, None, None, None))
                times = {}
                for name, call in (("call_ms", lambda: ctx.raw_stats(n)), ("nocopy_ms", without_copies)):
                    call(), call()
                    t = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        call()
                        t.append((time.perf_counter() - t0) * 1e3)
                    times[name] = [round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)]
                # the front end's undistortion of the same slots, by the library's stage timers
                ctx.mask_run(n)
                ctx.sync()
                ctx.set_stage_timing(True)
                ctx.stage_reset()
                for _ in range(5):
                    for at in range(0, n, 16):                          # (new rows: the front end runs again)
                        ctx.upload_frame_rows(frames[:min(16, n - at)], first=at)
                    ctx.mask_run(n)
                    ctx.sync()
                ms, launches = ctx.stage_ms()["undistort_rows"]
                ctx.set_stage_timing(False)
                case = {"format": fmt, "frame": content, "rows": list(rows), "bytes": nbytes, "call_ms_median_min_max": times["call_ms"],
                        "nocopy_ms_median_min_max": times["nocopy_ms"], "gbps_of_nocopy_ms": round(nbytes / times["nocopy_ms"][0] / 1e6, 1),
                        "undistort_rows_ms_per_batch": round(ms / 5, 4), "undistort_rows_launches_per_batch": launches / 5}
                print(json.dumps(case), flush=True)
                out["cases"].append(case)
        finally:
            ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
