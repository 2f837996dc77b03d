"""Shared helpers for the parity tests."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_files(prefix):
    return sorted(glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def unpack_mask(d):
    h, w = [int(v) for v in d["mask_shape"]]
    bits = np.unpackbits(d["mask_bits"])[: h * w].reshape(h, w)
    return (bits * int(d["mask_value"])).astype(np.uint8)


def params_of(d):
    return {k[len("param_"):]: d[k].item() for k in d.files if k.startswith("param_")}


# What lt_last_search_source reports for each search fixture once its mask has been uploaded as a bit plane (1: the bit-plane
# kernels ran; 0: the u8 kernels did -- band4's band is 2 * 60 + 2 columns, wider than the 64 a row mask holds).  Uploaded as
# bytes (lt_upload_masks) every one of them reports 0.
FIXTURE_BITS_SOURCE = {
    "sws_curvy.npz": 1, "sws_curvy_mu05.npz": 1, "sws_curvy_mu10.npz": 1, "sws_empty.npz": 1, "sws_lanes_noise0.npz": 1,
    "sws_lanes_noise1.npz": 1, "sws_lanes_noise2.npz": 1, "sws_lanes_noise3.npz": 1, "sws_left_edge.npz": 1, "sws_left_gap.npz": 1,
    "sws_limit3.npz": 1, "sws_limit50.npz": 1, "sws_nine_windows.npz": 1, "sws_no_left.npz": 1, "sws_no_right.npz": 1,
    "sws_odd_window.npz": 1, "sws_partial05.npz": 1, "sws_random1e4.npz": 1, "sws_random50.npz": 1, "sws_right_edge.npz": 1,
    "sws_right_gap.npz": 1, "sws_short_lines.npz": 1, "sws_small_img.npz": 1, "sws_solid_both.npz": 1, "sws_value1.npz": 1,
    "sws_wide_window.npz": 1,
    "band0.npz": 1, "band1.npz": 1, "band2.npz": 1, "band3.npz": 1, "band4.npz": 0, "band5.npz": 1, "band_halfint.npz": 1,
    "band_ignore0.npz": 1, "band_offimage.npz": 1, "band_random50.npz": 1,
}

def upload(c, masks, source, first=0):
    """the masks into the slots as bytes (lt_upload_masks) or as bit planes (lt_upload_mask_bits)"""
    return (c.upload_masks if source == "u8" else c.upload_mask_bits)(masks, first=first)


def search_source(source, bits_source):
    """What lt_last_search_source must say behind `upload(.., source)`: 0 for bytes, `bits_source` for bit planes -- unless the
    run forces the u8 or first-formulation kernels (the experiments build's switches: test_fallback_kernel_paths_...)."""
    forced = os.environ.get("LANE_TRACKER_AMD_LIB") and any(os.environ.get(k, "")[:1] == "1" for k in ("LT_SEARCH_U8", "LT_SWS_V1", "LT_BAND_V1"))
    if source == "u8" or forced:
        return 0
    return bits_source


def coeff_close(got, want, h=1100, tol=1e-4):
    """BASELINE tolerance: 1e-4 relative per coefficient with the absolute floor of SURVEY 8(a):
    |da| H^2, |db| H and |dc| each <= tol * max(1, |c|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    lim = tol * max(1.0, abs(float(want[2])))
    return (abs(got[0] - want[0]) * h * h <= lim and abs(got[1] - want[1]) * h <= lim
            and abs(got[2] - want[2]) <= lim)
