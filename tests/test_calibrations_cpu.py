"""Calibration sets without a GPU: what LaneTrackerGroup(calibrations=...) refuses before it touches the device, the new names at
the C boundary, and the test cameras themselves (tests/calibration_cameras.py) against the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import calibration_cameras as CC
from lane_tracker_amd import _native, group, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("lt_add_calibration", "lt_calibration_count", "lt_set_slot_calibrations", "lt_get_slot_calibrations", "lt_overlay_configure_set")


def test_new_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    lib = _native.load()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native._SIGNATURES and name in _native.exported_symbols() and hasattr(lib, name), name
    for method in ("add_calibration", "set_slot_calibrations", "slot_calibrations", "calibration_count"):
        assert callable(getattr(_native.Context, method))
    # the test hooks, which take planes or a fit by value: declared, exported and bound like everything else (additive: the ABI stays 5)
    for name, method in (("lt_lane_spans_from_fit", "lane_spans_from_fit"), ("lt_morph_ellipse", "morph_ellipse"), ("lt_morph_planes", "morph_planes")):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native._SIGNATURES and name in _native.exported_symbols() and hasattr(lib, name), name
        assert callable(getattr(_native.Context, method)), method
    # the header names every entry point that knows set 0 only
    for name in ("lt_present_frame", "lt_present_lane_async", "lt_present_lane_from_fit_async", "lt_present_finish", "lt_lane_spans_from_fit",
                 "lt_overlay_run_strip", "lt_overlay_run_strip_coeffs", "lt_search_viz_run", "lt_split_panes_run"):
        assert name in header.split("calibration sets: one context")[1].split("int  lt_add_calibration")[0], name


def test_null_arguments_are_errors_without_a_gpu():
    lib = _native.load()
    cal, i = _native.Calib(), C.c_int(0)
    ids = np.zeros(2, np.int32)
    assert lib.lt_add_calibration(None, C.byref(cal), C.byref(i)) == -1
    assert lib.lt_calibration_count(None, C.byref(i)) == -1
    assert lib.lt_set_slot_calibrations(None, 0, 2, ids.ctypes.data) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_get_slot_calibrations(None, 0, 2, ids.ctypes.data) == -1
    assert lib.lt_overlay_configure_set(None, 1, np.eye(3).ctypes.data) == -1


def test_a_wrong_calibrations_argument_is_refused_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(_native, "Context", no_device)
    cams = CC.cameras()
    ref, b = cams["A"], CC.overrides(cams["B"])
    for bad, exc in (([None, b], ValueError), ([None, b, None, None], ValueError), ([None, dict(b, focal=1.0), None], ValueError),
                     ([None, dict(img_size=(1280, 720)), None], ValueError), ([None, 3, None], TypeError),
                     ([None, dict(warp_matrices=(np.eye(3),)), None], ValueError)):
        with pytest.raises(exc):
            group.LaneTrackerGroup(3, **ref, calibrations=bad)
    with pytest.raises(AssertionError, match="device context"):
        group.LaneTrackerGroup(3, **ref, calibrations=[None, b, {}])      # a good list gets as far as the device
    with pytest.raises(TypeError):
        group.LaneTrackerGroup(3, ref["img_size"], ref["warped_size"], ref["cam_matrix"], ref["dist_coeffs"], ref["warp_matrices"],
                               ref["mpp_conversion"], 8, 4, 2, False, 0, [None] * 3)                       # keyword only


def test_streams_with_equal_arrays_share_a_key():
    cams = CC.cameras()
    own = dict(cams["A"])
    full = group._stream_calibrations([None, {}, dict(cam_matrix=own["cam_matrix"].copy()), CC.overrides(cams["C"]),
                                       dict(mpp_conversion=(1.0, 2.0))], 5, CC.overrides(own))
    keys = [group._table_key(c) for c in full]
    assert keys[0] == keys[1] == keys[2] == keys[4] != keys[3]
    assert full[4]["mpp_conversion"] == (1.0, 2.0) and full[3]["dist_coeffs"] is not own["dist_coeffs"]
    assert len({group._table_key(CC.overrides(c)) for c in cams.values()}) == 5


def test_the_shift_of_camera_b_moves_the_scene():
    f = np.arange(2 * 6 * 8 * 3, dtype=np.uint8).reshape(2, 6, 8, 3)
    g = CC.shifted(f, (3, -2))
    assert np.array_equal(g[:, :4, 3:], f[:, 2:, :5]) and not g[:, 4:].any() and not g[:, :, :3].any()
    assert np.array_equal(CC.shifted(f, (-1, 1))[:, 1:, :7], f[:, :5, 1:])


@pytest.mark.parametrize("name", CC.NAMES)
def test_the_oracle_accepts_the_lane_of_every_test_camera(oracle, name):
    cam = CC.cameras()[name]
    oc = CC.oracle_calib(oracle, cam)
    assert oracle.warp_source_rows(oc) == ((447, 685) if name == "B" else (457, 695))
    renderer = synth.SceneRenderer()
    for scene in range(8):
        r = oracle.frame_sws_fit(oc, CC.frames_for(name, renderer.render(scene)[0]), fast=True)
        assert r["detected"] and oracle.check_validity(cam["warped_size"], r["coeffs"][0], r["coeffs"][1]), (name, scene)
