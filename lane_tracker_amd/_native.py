"""ctypes binding of liblane_tracker_amd.so (include/lane_tracker_amd.h).

The library is HIP-only.  There is deliberately no fallback: if the shared object is missing or no
GPU is visible, constructing a `Context` raises -- nothing in this package computes on the CPU.
"""
import ctypes as C
import math
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LANE_TRACKER_AMD_LIB: load another build of the same library (tools/toolchain_cases.sh compares variant builds)
LIB_PATH = os.environ.get("LANE_TRACKER_AMD_LIB") or os.path.join(_HERE, "liblane_tracker_amd.so")
NUM_STAGES = 12
ABI_VERSION = 5          # LT_ABI_VERSION of include/lane_tracker_amd.h this table was written against

PLANE_R, PLANE_LAB_B, PLANE_TOPHAT_R, PLANE_TOPHAT_B, PLANE_MERGED, PLANE_MASK = range(6)


class NativeError(RuntimeError):
    pass


class Calib(C.Structure):
    _fields_ = [("img_w", C.c_int32), ("img_h", C.c_int32), ("warp_w", C.c_int32), ("warp_h", C.c_int32),
                ("cam_matrix", C.c_double * 9), ("dist_coeffs", C.c_double * 5), ("M", C.c_double * 9)]


class FilterParams(C.Structure):
    _fields_ = [("filter_type", C.c_int32), ("ksize_r", C.c_int32), ("C_r", C.c_int32), ("ksize_b", C.c_int32),
                ("C_b", C.c_int32), ("mask_noise", C.c_int32), ("noise_thresh", C.c_int32),
                ("ksize_noise", C.c_int32), ("C_noise", C.c_int32)]


class SearchParams(C.Structure):
    _fields_ = [("window_width", C.c_int32), ("window_height", C.c_int32), ("search_range", C.c_int32),
                ("no_success_limit", C.c_int32), ("ignore_sides", C.c_int32), ("ignore_bottom", C.c_int32),
                ("bandwidth", C.c_int32), ("_pad", C.c_int32), ("mu", C.c_double), ("start_slice", C.c_double),
                ("partial", C.c_double)]


class LaneRecord(C.Structure):
    _fields_ = [("left_coeffs", C.c_double * 3), ("right_coeffs", C.c_double * 3), ("n_left", C.c_int32),
                ("n_right", C.c_int32), ("detected", C.c_uint8), ("fit_flags", C.c_uint8), ("mode", C.c_uint8),
                ("_pad", C.c_uint8), ("frame", C.c_int32)]


RECORD_DTYPE = np.dtype([("left_coeffs", "<f8", 3), ("right_coeffs", "<f8", 3), ("n_left", "<i4"),
                         ("n_right", "<i4"), ("detected", "u1"), ("fit_flags", "u1"), ("mode", "u1"),
                         ("_pad", "u1"), ("frame", "<i4")])
assert RECORD_DTYPE.itemsize == 64 and C.sizeof(LaneRecord) == 64


class SearchItem(C.Structure):
    """lt_search_item: one frame of lt_search_fit_list (slot, 0 sliding window / 1 band, the band's prior coefficients)."""
    _fields_ = [("slot", C.c_int32), ("mode", C.c_int32), ("_pad", C.c_int32 * 2), ("prev_coeffs", C.c_double * 6)]


SEARCH_ITEM_DTYPE = np.dtype([("slot", "<i4"), ("mode", "<i4"), ("_pad", "<i4", 2), ("prev_coeffs", "<f8", 6)])
assert SEARCH_ITEM_DTYPE.itemsize == 64 and C.sizeof(SearchItem) == 64


class VizItem(C.Structure):
    """lt_viz_item: one frame of lt_search_viz_run / lt_split_panes_run (slot, 0 bare mask / 1 sliding window / 2 band, the shown
    search's parameters, the lengths of the frame's stretches of the four point lists)."""
    _fields_ = [("slot", C.c_int32), ("kind", C.c_int32), ("window_width", C.c_int32), ("window_height", C.c_int32),
                ("ignore_bottom", C.c_int32), ("bandwidth", C.c_int32), ("n_fit_left", C.c_int32), ("n_fit_right", C.c_int32),
                ("n_band_left", C.c_int32), ("n_band_right", C.c_int32), ("_pad", C.c_int32 * 2)]


VIZ_ITEM_DTYPE = np.dtype([("slot", "<i4"), ("kind", "<i4"), ("window_width", "<i4"), ("window_height", "<i4"), ("ignore_bottom", "<i4"),
                           ("bandwidth", "<i4"), ("n_fit_left", "<i4"), ("n_fit_right", "<i4"), ("n_band_left", "<i4"),
                           ("n_band_right", "<i4"), ("_pad", "<i4", 2)])
assert VIZ_ITEM_DTYPE.itemsize == 48 and C.sizeof(VizItem) == 48
VIZ_MASK, VIZ_SWS, VIZ_BAND = 0, 1, 2


class DeviceSurface(C.Structure):
    """lt_device_surface: one camera frame in device memory (plane pointers, luma / RGB pitch, chroma pitch)."""
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_int32), ("chroma_pitch", C.c_int32)]


SURFACE_DTYPE = np.dtype([("plane", "<u8", 3), ("pitch", "<i4"), ("chroma_pitch", "<i4")])
assert SURFACE_DTYPE.itemsize == 32 and C.sizeof(DeviceSurface) == 32


class Info(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("capacity", C.c_int32),
                ("cu_count", C.c_int32), ("src_row0", C.c_int32), ("src_row1", C.c_int32),
                ("max_pixels_per_side", C.c_int32), ("max_levels", C.c_int32), ("alg_bytes_mask", C.c_int64),
                ("alg_bytes_search", C.c_int64), ("device_name", C.c_char * 64)]


class RawStatsParams(C.Structure):
    """lt_raw_stats_params: the rectangle, the zone grid and the validity bounds (by colour phase) of a statistics call."""
    _fields_ = [("row0", C.c_int32), ("row1", C.c_int32), ("col0", C.c_int32), ("col1", C.c_int32), ("grid_h", C.c_int32), ("grid_w", C.c_int32),
                ("lo", C.c_int32 * 4), ("hi", C.c_int32 * 4)]


# name -> (restype, argtypes); every symbol include/lane_tracker_amd.h declares
_P = C.c_void_p
_SIGNATURES = {
    "lt_last_error": (C.c_char_p, []),
    "lt_abi_version": (C.c_int, []),
    "lt_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "lt_create": (C.c_int, [C.POINTER(Calib), C.c_int, C.POINTER(_P)]),
    "lt_destroy": (None, [_P]),
    "lt_reserve": (C.c_int, [_P, C.c_int]),
    "lt_get_info": (C.c_int, [_P, C.POINTER(Info)]),
    "lt_sync": (C.c_int, [_P]),
    "lt_set_streams": (C.c_int, [_P, C.c_int]),
    "lt_upload_frames": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_get_source_rows": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lt_upload_frame_rows": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_upload_frame_rows_async": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_upload_frame_rows_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_upload_frame_rest": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_upload_frame_rest_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "lt_upload_masks": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_upload_mask_bits": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_download_masks": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_download_plane": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "lt_download_undistorted": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_download_records": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_download_pixels": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int, C.POINTER(C.c_int)]),
    "lt_download_centroids": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.POINTER(C.c_int)]),
    "lt_download_lane_lists": (C.c_int, [_P, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int,
                               C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "lt_copy_records_to_device": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_enqueue_records_to_device": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_overlay_configure": (C.c_int, [_P, _P]),
    "lt_overlay_run": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_double]),
    "lt_overlay_set_font": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "lt_overlay_text": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "lt_overlay_rows": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lt_present_frame": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_double, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "lt_present_lane_async": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_double, _P, _P]),
    "lt_present_finish": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "lt_overlay_run_strip_coeffs": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_double]),
    "lt_present_lane_from_fit_async": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_double, _P, _P]),
    "lt_lane_spans_from_fit": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_int, _P]),
    "lt_lane_polygon_spans": (C.c_int, [C.c_int, _P, C.c_int, _P, C.c_int, _P]),
    "lt_download_overlay": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_download_overlay_async": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_download_bev": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_search_viz_run": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    "lt_split_panes_run": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    "lt_split_panes_size": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lt_search_viz_wait": (C.c_int, [_P]),
    "lt_calib_split_panes_size": (C.c_int, [C.POINTER(Calib), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lt_resize_linear_u8": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "lt_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "lt_host_free": (C.c_int, [_P]),
    "lt_host_copy_async": (C.c_int, [_P, _P, C.c_size_t]),
    "lt_host_copy2d_async": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t]),
    "lt_overlay_run_rows": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_double, _P]),
    "lt_download_overlay_rows_async": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "lt_host_copy_wait": (C.c_int, []),
    "lt_host_copy_group_create": (C.c_int, [C.POINTER(C.c_int)]),
    "lt_host_copy_group_destroy": (C.c_int, [C.c_int]),
    "lt_host_copy_async_group": (C.c_int, [C.c_int, _P, _P, C.c_size_t]),
    "lt_host_copy2d_async_group": (C.c_int, [C.c_int, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t]),
    "lt_host_copy_wait_group": (C.c_int, [C.c_int]),
    "lt_host_touch_async_group": (C.c_int, [C.c_int, _P, C.c_size_t]),
    "lt_shutdown": (C.c_int, []),
    "lt_host_copy_stats": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "lt_warm": (C.c_int, [_P, C.POINTER(SearchParams), C.POINTER(SearchParams), C.c_int]),
    "lt_overlay_run_strip": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_double]),
    "lt_strip_download_async": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t, C.c_int]),
    "lt_text_blend_host": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_int]),
    "lt_host_text_async_group": (C.c_int, [C.c_int, _P, C.c_size_t, _P, C.c_size_t, C.c_int, _P, C.c_int, C.c_int, _P, _P,
                                           C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "lt_host_text_now_group": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int]),
    "lt_mask_run": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(FilterParams)]),
    "lt_mask_rerun": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(FilterParams)]),
    "lt_upload_bev": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_filter_run": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(FilterParams)]),
    "lt_sws_fit_run": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(SearchParams)]),
    "lt_band_fit_run": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(SearchParams), _P]),
    "lt_search_fit_list": (C.c_int, [_P, C.c_int, _P, C.POINTER(SearchParams), C.POINTER(SearchParams)]),
    "lt_upload_frame_rows_list": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_upload_frame_rest_list": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_band_fit_chain_run": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(SearchParams), _P]),
    "lt_band_fit_chain_collect": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_band_fit_chain_cancel": (C.c_int, [_P]),
    "lt_set_search_cus": (C.c_int, [_P, C.c_int]),
    "lt_set_walk_min_frames": (C.c_int, [_P, C.c_int]),
    "lt_set_direct_upload": (C.c_int, [_P, C.c_int]),
    "lt_direct_upload_count": (C.c_ulonglong, [_P]),
    "lt_set_urgent": (C.c_int, [_P, C.c_int]),
    "lt_poly_points": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P]),
    "lt_frame_tail": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P]),
    "lt_download_overlay_wait": (C.c_int, [_P]),
    "lt_set_frame_base": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "lt_mask_batch": (C.c_int, [_P, _P, C.c_int, C.POINTER(FilterParams), _P]),
    "lt_sws_fit_batch": (C.c_int, [_P, _P, C.c_int, C.POINTER(SearchParams), _P]),
    "lt_band_fit_batch": (C.c_int, [_P, _P, C.c_int, C.POINTER(SearchParams), _P, _P]),
    "lt_bilateral_adaptive_threshold": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, _P]),
    "lt_filter_lane_points": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(FilterParams), _P]),
    "lt_morph_ellipse": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "lt_morph_planes": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "lt_fit_poly2": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "lt_calib_source_rows": (C.c_int, [C.POINTER(Calib), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lt_calib_warp_table": (C.c_int, [C.POINTER(Calib), _P, _P]),
    "lt_calib_undistort_table": (C.c_int, [C.POINTER(Calib), C.c_int, C.c_int, _P, _P]),
    "lt_calib_lab_tables": (C.c_int, [_P, _P, _P]),
    "lt_calib_ellipse": (C.c_int, [C.c_int, _P, C.POINTER(C.c_int)]),
    "lt_gather_init": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(_P)]),
    "lt_gather_world": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lt_gather_reserve": (C.c_int, [_P, C.c_int]),
    "lt_gather_stage": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "lt_gather_records": (C.c_int, [_P, C.c_int, _P]),
    "lt_gather_host": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "lt_gather_barrier": (C.c_int, [_P]),
    "lt_gather_destroy": (None, [_P]),
    "lt_timer_start": (C.c_int, [_P]),
    "lt_timer_stop": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "lt_set_stage_timing": (C.c_int, [_P, C.c_int]),
    "lt_stage_reset": (C.c_int, [_P]),
    "lt_stage_ms": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int]),
    "lt_stage_name": (C.c_char_p, [C.c_int]),
    "lt_device_cache_trim": (C.c_int, [C.c_size_t]),
    "lt_device_cache_stats": (C.c_int, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "lt_device_cache_counters": (C.c_int, [C.POINTER(C.c_ulonglong)] * 4),
    "lt_host_memory_stats": (C.c_int, [C.POINTER(C.c_size_t)] * 3),
    "lt_set_download_method": (C.c_int, [_P, C.c_int]),
    "lt_download_stats": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "lt_last_threshold_path": (C.c_int, [_P]),
    "lt_last_threshold_form": (C.c_int, [_P]),
    "lt_last_open_form": (C.c_int, [_P]),
    "lt_last_tophat_path": (C.c_int, [_P]),
    "lt_last_search_source": (C.c_int, [_P]),
    "lt_tophat_split_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "lt_last_adaptive_path": (C.c_int, [_P]),
    "lt_set_input_format": (C.c_int, [_P, C.c_int, _P]),
    "lt_get_input_format": (C.c_int, [_P, C.POINTER(C.c_int), _P]),
    "lt_set_input_size": (C.c_int, [_P, C.c_int, C.c_int]),
    "lt_get_input_size": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lt_get_input_rows": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lt_yuv_to_rgb": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "lt_bayer_to_rgb": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "lt_set_raw_lut": (C.c_int, [_P, _P]),
    "lt_get_raw_lut": (C.c_int, [_P, _P, C.POINTER(C.c_int)]),
    "lt_set_raw_lut_wide": (C.c_int, [_P, _P, C.c_size_t]),
    "lt_get_raw_lut_wide": (C.c_int, [_P, _P, C.c_size_t]),
    "lt_raw16_to_rgb": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "lt_set_raw_color": (C.c_int, [_P, _P, _P, C.c_int]),
    "lt_get_raw_color": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int)]),
    "lt_raw_to_rgb_color": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, _P]),
    "lt_set_raw_shading": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int]),
    "lt_get_raw_shading": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), _P, C.POINTER(C.c_int)]),
    "lt_get_raw_shading_plane": (C.c_int, [_P, _P]),
    "lt_raw_to_rgb_shaded": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "lt_raw_stats": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(RawStatsParams), _P, _P, _P, _P]),
    "lt_attach_device_frames": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "lt_device_frames_rest": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_device_alloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]),
    "lt_device_free": (C.c_int, [_P]),
    "lt_device_write": (C.c_int, [_P, _P, C.c_size_t]),
    "lt_device_read": (C.c_int, [_P, _P, C.c_size_t]),
    "lt_device_stream_wait": (C.c_int, [C.c_int, C.c_size_t]),
    "lt_rgb_to_surfaces": (C.c_int, [C.c_int, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "lt_overlay_store_device": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P]),
    "lt_overlay_store_wait": (C.c_int, [_P]),
    "lt_overlay_run_inplace": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_double, _P, _P]),
    "lt_overlay_run_to_surfaces": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_double, _P, _P, C.c_int, _P]),
    "lt_last_overlay_launches": (C.c_int, [_P]),
    "lt_overlay_run_inplace_coeffs": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_double, _P, _P]),
    "lt_add_calibration": (C.c_int, [_P, C.POINTER(Calib), C.POINTER(C.c_int)]),
    "lt_calibration_count": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lt_set_slot_calibrations": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_get_slot_calibrations": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_overlay_configure_set": (C.c_int, [_P, C.c_int, _P]),
    "lt_add_raw_set": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lt_raw_set_count": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lt_set_slot_raw_sets": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_get_slot_raw_sets": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "lt_set_raw_lut_of": (C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    "lt_get_raw_lut_of": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.POINTER(C.c_int)]),
    "lt_set_raw_color_of": (C.c_int, [_P, C.c_int, _P, _P, C.c_int]),
    "lt_get_raw_color_of": (C.c_int, [_P, C.c_int, _P, _P, C.POINTER(C.c_int)]),
    "lt_set_raw_shading_of": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int]),
    "lt_get_raw_shading_of": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), _P, C.POINTER(C.c_int)]),
    "lt_get_raw_shading_plane_of": (C.c_int, [_P, C.c_int, _P]),
    "lt_last_raw_walk_form": (C.c_int, [_P]),
}

# camera-frame formats (lt_input_layout) and the conversion matrices {CY, CVR, CVG, CUG, CUB} of include/lane_tracker_amd.h
# PIXEL_FORMATS is the SINK-CAPABLE SUBSET -- what a camera frame and a destination of annotated frames can both be -- and not the list
# of formats a camera can have: that is INPUT_FORMATS, which adds packed 4:2:2 (one plane of (H, W, 2) bytes; camera frames only).
PIXEL_FORMATS = {"rgb": 0, "nv12": 1, "i420": 2}
INPUT_FORMATS = dict(PIXEL_FORMATS, yuy2=3, uyvy=4)                # every format a camera frame can have (pixel_format_id)
PACKED_422 = ("yuy2", "uyvy")                                      # the names INPUT_FORMATS adds
# ... and the RGB family's other members, as users' own software holds frames: 'bgr' (H, W, 3) -- OpenCV's order --, 'rgba' / 'bgra'
# (H, W, 4), alpha never read.  A channel permutation, no conversion; camera frames AND sinks (alpha written as 255).  A table of
# its own: the three above keep their contents.
RGB_FAMILY = {"bgr": 5, "rgba": 6, "bgra": 7}
# ... and 8-bit raw Bayer, as a sensor delivers it before any image signal processor: one plane of (H, W) bytes, named by the
# sensor's top-left 2 x 2 block; demosaiced (bilinear) on the device.  Camera frames only.  Again a table of its own.
BAYER_FORMATS = {"bayer_rggb": 16, "bayer_grbg": 17, "bayer_gbrg": 18, "bayer_bggr": 19}
# ... and 10- / 12-bit raw Bayer, as most raw sensors deliver it: one plane of (H, W) uint16 -- the sample in the low 10 / 12 bits of a
# little-endian 16-bit word, the bits above ignored -- looked up in a table u8 (4, 2**bits) on the device (utils.raw_lut(bits=..)), then
# the 8-bit demosaic.  The pattern is id & 3, in BAYER_FORMATS' order.  Camera frames only; once more a table of its own.
BAYER_WIDE_FORMATS = {"bayer10_rggb": 32, "bayer10_grbg": 33, "bayer10_gbrg": 34, "bayer10_bggr": 35,
                      "bayer12_rggb": 48, "bayer12_grbg": 49, "bayer12_gbrg": 50, "bayer12_bggr": 51}
# ... and the same samples MIPI-packed, as a CSI-2 receiver writes them (V4L2 SRGGB10P / SRGGB12P ...): one plane of bytes, (H, W * 5 // 4) --
# five bytes for four samples, W % 4 == 0 -- or (H, W * 3 // 2) -- three bytes for two --, unpacked in the kernels (utils.pack_raw /
# unpack_raw are the definition).  id = the 16-bit format's | 4.  Table, colour stage and shading map as for BAYER_WIDE_FORMATS.
BAYER_PACKED_FORMATS = {"bayer10p_rggb": 36, "bayer10p_grbg": 37, "bayer10p_gbrg": 38, "bayer10p_bggr": 39,
                        "bayer12p_rggb": 52, "bayer12p_grbg": 53, "bayer12p_gbrg": 54, "bayer12p_bggr": 55}
# every raw format whose samples have more than 8 bits: behind a wide table u8 (4, 2**bits)
BAYER_DEEP_FORMATS = dict(BAYER_WIDE_FORMATS, **BAYER_PACKED_FORMATS)
RAW_FORMATS = dict(BAYER_FORMATS, **BAYER_DEEP_FORMATS)
YUV_MATRICES = {"bt601": (1220542, 1673527, -852492, -409993, 2116026),
                "bt709": (1220542, 1880097, -558891, -223347, 2214593)}


# ... and the way out, RGB -> YUV 4:2:0 {CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV} (LT_RGB2YUV_BT601 / _BT709)
RGB2YUV_MATRICES = {"bt601": (269484, 528482, 102760, -155188, -305135, 460324, -385875, -74448),
                    "bt709": (191455, 644067, 65019, -105533, -355018, 460551, -418321, -42230)}


class InplaceText(C.Structure):
    """lt_inplace_text: the text lines of an in-place draw."""
    _fields_ = [("lines", C.c_char_p), ("n_lines", C.c_int32), ("line_len", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("step", C.c_int32)]


def rgb2yuv_coeffs(matrix):
    """'bt601' / 'bt709', or eight integers {CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV} -> the int32 array the library takes."""
    if isinstance(matrix, str):
        if matrix not in RGB2YUV_MATRICES:
            raise ValueError("matrix must be 'bt601' or 'bt709', got %r" % (matrix,))
        matrix = RGB2YUV_MATRICES[matrix]
    k = np.ascontiguousarray(matrix, dtype=np.int32)
    if k.shape != (8,):
        raise ValueError("an RGB -> YUV matrix is eight integers")
    return k


def rgb_to_surfaces(rgb_ptr, frame_stride, img_size, sink, matrix="bt601", device=0):
    """len(sink) dense RGB frames of `img_size` at device address `rgb_ptr` (a block of lt_device_alloc), `frame_stride` bytes
    apart -> the surfaces of `sink` (a device.DeviceFrames), in its pixel format (lt_rgb_to_surfaces); synchronous."""
    layout = sink_format_id(sink.pixel_format)
    k = rgb2yuv_coeffs(matrix) if is_yuv(layout) else None
    s = np.ascontiguousarray(sink.surfaces)
    _check(load().lt_rgb_to_surfaces(int(device), C.c_void_p(int(rgb_ptr)), int(frame_stride), int(img_size[1]), int(img_size[0]), s.shape[0],
                                     s.ctypes.data, layout, None if k is None else k.ctypes.data))


def raw_bits(pixel_format):
    """The sample bits of a raw Bayer format: 8, 10 or 12; 0 for every other format."""
    if pixel_format in BAYER_DEEP_FORMATS:
        return 10 if BAYER_DEEP_FORMATS[pixel_format] < 48 else 12
    return 8 if pixel_format in BAYER_FORMATS else 0


def packed_row_bytes(pixel_format, w):
    """The bytes of a row of `w` samples of a MIPI-packed raw format: w * 5 // 4 (RAW10) or w * 3 // 2 (RAW12)."""
    return int(w) * 5 // 4 if raw_bits(pixel_format) == 10 else int(w) * 3 // 2


def unpacked_format(pixel_format):
    """'bayer10p_rggb' -> 'bayer10_rggb': the 16-bit format of a MIPI-packed one's samples (any other name: itself)."""
    return pixel_format.replace("p_", "_", 1) if pixel_format in BAYER_PACKED_FORMATS else pixel_format


def raw_frame_size(a, pattern):
    """(h, w) of the raw Bayer frame `a` -- (H, W), or (H, row bytes) for a MIPI-packed pattern --, ValueError where that is no legal size."""
    if pattern in BAYER_PACKED_FORMATS:
        per, of = (5, 4) if raw_bits(pattern) == 10 else (3, 2)
        if a.ndim != 2 or a.shape[1] % per or a.shape[0] % 2 or a.shape[0] < 4 or a.shape[1] * of // per < 4:
            raise ValueError("a MIPI-packed %r frame is a 2-D uint8 array of shape (H, W * %d // %d) with H even, W a multiple of %d and both at "
                             "least 4, got %r" % (pattern, per, of, of, a.shape))
        return a.shape[0], a.shape[1] * of // per
    if a.ndim != 2 or a.shape[0] % 2 or a.shape[1] % 2 or a.shape[0] < 4 or a.shape[1] < 4:
        raise ValueError("a raw Bayer frame is a 2-D array of shape (H, W) with H and W even and at least 4, got %r" % (a.shape,))
    return a.shape[0], a.shape[1]


def frame_dtype(pixel_format):
    """The dtype of a camera frame in `pixel_format`: uint16 for 10- / 12-bit raw Bayer in words, uint8 for everything else (MIPI-packed
    10- / 12-bit raw Bayer included)."""
    return np.dtype(np.uint16) if pixel_format in BAYER_WIDE_FORMATS else np.dtype(np.uint8)


def frames_array(frames, pixel_format):
    """`frames` as a C-contiguous array of the format's dtype.  Between uint8 and uint16 nothing is cast: uint8 frames handed to a 10- /
    12-bit raw Bayer tracker, and uint16 frames handed to any other, are a ValueError."""
    want = frame_dtype(pixel_format)
    have = getattr(frames, "dtype", None)
    if have is not None and have != want and (want == np.uint16 or have == np.uint16):
        raise ValueError("pixel_format=%r takes %s camera frames, got %s" % (pixel_format, want, have))
    return np.ascontiguousarray(frames, want)


def pixel_format_id(pixel_format):
    try:
        if pixel_format in INPUT_FORMATS:
            return INPUT_FORMATS[pixel_format]
        if pixel_format in BAYER_DEEP_FORMATS:
            return BAYER_DEEP_FORMATS[pixel_format]
        return RGB_FAMILY[pixel_format] if pixel_format in RGB_FAMILY else BAYER_FORMATS[pixel_format]
    except (KeyError, TypeError):
        raise ValueError("pixel_format must be 'rgb', 'nv12', 'i420', 'yuy2', 'uyvy', 'bgr', 'rgba', 'bgra' or 'bayer_rggb' / '_grbg' / '_gbrg' / "
                         "'_bggr' (10 / 12 bits: 'bayer10_*' / 'bayer12_*'; MIPI-packed: 'bayer10p_*' / 'bayer12p_*'), got %r" % (pixel_format,)) from None


def format_name(layout):
    """The name of an lt_input_layout value."""
    return {v: n for n, v in list(INPUT_FORMATS.items()) + list(RGB_FAMILY.items()) + list(BAYER_FORMATS.items()) +
            list(BAYER_DEEP_FORMATS.items())}[int(layout)]


def is_yuv(layout):
    """Does an lt_input_layout value name a YUV format (one that is converted with a matrix)?"""
    return 1 <= int(layout) <= 4


def sink_format_id(pixel_format):
    """pixel_format_id for a destination of annotated frames: packed 4:2:2 and raw Bayer are input formats only."""
    if pixel_format in PACKED_422 or pixel_format in RAW_FORMATS:
        raise ValueError("%r is an input format only: annotated frames go into 'rgb', 'bgr', 'rgba', 'bgra', 'nv12' or 'i420' surfaces" % (pixel_format,))
    return pixel_format_id(pixel_format)


def draw_sink_format_id(pixel_format):
    """sink_format_id for the one-launch draw into sinks (lt_overlay_run_to_surfaces, a LaneTrackerGroup's `out=`): 'rgb', 'nv12' or
    'i420' only."""
    if pixel_format in RGB_FAMILY:
        raise ValueError("a group's out= sink is 'rgb', 'nv12' or 'i420': %r sinks are written by a tracker's process_batch / process_stream" % (pixel_format,))
    return sink_format_id(pixel_format)


def yuv_coeffs(matrix):
    """'bt601' / 'bt709', or five integers {CY, CVR, CVG, CUG, CUB} -> the int32 array the library takes."""
    if isinstance(matrix, str):
        if matrix not in YUV_MATRICES:
            raise ValueError("yuv_matrix must be 'bt601' or 'bt709', got %r" % (matrix,))
        matrix = YUV_MATRICES[matrix]
    k = np.ascontiguousarray(matrix, dtype=np.int32)
    if k.shape != (5,):
        raise ValueError("a conversion matrix is five integers")
    return k


def checked_raw_lut(raw_lut, pixel_format):
    """`raw_lut` of a tracker or group as the u8 (4, 256) array the device takes, or None; ValueError -- before any device call -- for a
    table with a pixel format that is not raw Bayer, for another shape or another dtype."""
    if raw_lut is None:
        return None
    from .utils import checked_raw_lut as _checked
    if pixel_format in BAYER_DEEP_FORMATS:               # u8 (4, 2**bits)
        return _checked(raw_lut, raw_bits(pixel_format))
    if pixel_format not in BAYER_FORMATS:
        raise ValueError("raw_lut conditions raw Bayer frames: pixel_format=%r takes none" % (pixel_format,))
    return _checked(raw_lut)


def effective_raw_lut(raw_lut, pixel_format):
    """checked_raw_lut, and for the 10- / 12-bit formats -- which always have a table -- the default `utils.raw_lut(bits=..)` for None."""
    lut = checked_raw_lut(raw_lut, pixel_format)
    if lut is None and pixel_format in BAYER_DEEP_FORMATS:
        from .utils import raw_lut as _default
        lut = _default(bits=raw_bits(pixel_format))
    return lut


def checked_raw_color(ccm, curve, pixel_format):
    """`raw_ccm` / `raw_curve` of a tracker or group as the int16 (3, 3) and u8 (256,) arrays the device takes (None stays None);
    ValueError -- before any device call -- for a stage with a pixel format that is not raw Bayer, and for another shape or dtype."""
    if ccm is None and curve is None:
        return None, None
    from .utils import checked_raw_ccm, checked_raw_curve
    if pixel_format not in RAW_FORMATS:
        raise ValueError("raw_ccm / raw_curve follow the demosaic of raw Bayer frames: pixel_format=%r takes none" % (pixel_format,))
    return (None if ccm is None else checked_raw_ccm(ccm)), (None if curve is None else checked_raw_curve(curve))


def checked_raw_shading(shading, pixel_format):
    """`raw_shading` of a tracker or group as the utils.RawShading (mesh uint16 (4, mh, mw), black int32 (4,)) the device takes, or None;
    ValueError -- before any device call -- for a map with a pixel format that is not raw Bayer, for a mesh of another shape or dtype
    and for a black value above the format's largest sample."""
    if shading is None:
        return None
    from .utils import checked_raw_shading as _checked
    if pixel_format not in RAW_FORMATS:
        raise ValueError("raw_shading corrects raw Bayer frames: pixel_format=%r takes none" % (pixel_format,))
    return _checked(shading, raw_bits(pixel_format))


def default_stats_rows(input_rows):
    """The default rows of a statistics call: the run (r0, r1) the uploads bring (`Context.input_rows`), rounded inward to even."""
    return (int(input_rows[0]) + 1) & ~1, int(input_rows[1]) & ~1


def checked_raw_stats(pixel_format, img_size, input_rows, grid=(8, 8), rows=None, cols=None, lo=None, hi=None):
    """The arguments of `Context.raw_stats` / `LaneTracker.raw_stats` as the lt_raw_stats_params the library takes -- the rectangle written
    out, never the defaults' zeros; ValueError -- before any device call -- for a pixel format that is not raw Bayer, odd, empty or
    out-of-frame bounds, a grid side outside 1 .. 64 or above the rectangle's cells, a bound outside 0 .. 2**bits - 1.  `input_rows`: the run
    the uploads bring (`Context.input_rows()`), whose inward rounding to even rows is the default for rows=None."""
    if pixel_format not in RAW_FORMATS:
        raise ValueError("raw statistics are taken of raw Bayer frames: pixel_format=%r has none" % (pixel_format,))
    from .utils import checked_raw_stats_args
    r, c, g, lo, hi = checked_raw_stats_args(img_size, raw_bits(pixel_format), default_stats_rows(input_rows), grid, rows, cols, lo, hi)
    return RawStatsParams(r[0], r[1], c[0], c[1], g[0], g[1], (C.c_int32 * 4)(*[int(v) for v in lo]), (C.c_int32 * 4)(*[int(v) for v in hi]))


def checked_input_size(input_size, img_size, pixel_format="rgb"):
    """`input_size` = (width, height) of the frames a tracker is fed when that is not its calibration's `img_size`, as a tuple of two
    ints, or None (no input size, or the calibration's own); ValueError for a size outside 1 .. 16384 and for YUV frames."""
    if input_size is None:
        return None
    try:
        w, h = (int(v) for v in input_size)
    except (TypeError, ValueError):
        raise ValueError("input_size is (width, height), got %r" % (input_size,)) from None
    if not (1 <= w <= 16384 and 1 <= h <= 16384):
        raise ValueError("input_size must be 1 .. 16384 pixels wide and high, got %dx%d" % (w, h))
    if (w, h) == (int(img_size[0]), int(img_size[1])):
        return None
    pixel_format_id(pixel_format)
    if pixel_format != "rgb":
        raise ValueError("input_size resizes RGB frames only: pixel_format=%r frames must come in the calibration's size" % (pixel_format,))
    return w, h


def frame_shape(img_size, pixel_format="rgb"):
    """Shape of one camera frame of `img_size` = (width, height) in `pixel_format`: (H, W, 3), (H * 3 // 2, W) for 4:2:0, or
    (H, W, 2) for packed 4:2:2 (OpenCV's CV_8UC2); 'bgr': (H, W, 3), 'rgba' / 'bgra': (H, W, 4); raw Bayer: (H, W), MIPI-packed
    (H, W * 5 // 4) / (H, W * 3 // 2) bytes."""
    w, h = int(img_size[0]), int(img_size[1])
    if pixel_format_id(pixel_format) == 0:
        return (h, w, 3)
    if pixel_format in RGB_FAMILY:
        if w < 1 or h < 1:
            raise ValueError("empty %r frames: %dx%d" % (pixel_format, w, h))
        return (h, w, 3 if pixel_format == "bgr" else 4)
    if pixel_format in RAW_FORMATS:
        if w % 2 or h % 2 or w < 4 or h < 4:
            raise ValueError("raw Bayer frames need an even width and height of at least 4, got %dx%d" % (w, h))
        if pixel_format in BAYER_PACKED_FORMATS:
            if raw_bits(pixel_format) == 10 and w % 4:
                raise ValueError("MIPI-packed RAW10 frames need a width that is a multiple of 4, got %dx%d" % (w, h))
            return (h, packed_row_bytes(pixel_format, w))
        return (h, w)
    if pixel_format in PACKED_422:
        if w % 2 or w < 4 or h < 1:
            raise ValueError("4:2:2 frames need an even width of at least 4, got %dx%d" % (w, h))
        return (h, w, 2)
    if w % 2 or h % 2:
        raise ValueError("4:2:0 frames need an even width and height, got %dx%d" % (w, h))
    return (h * 3 // 2, w)



def input_frame_shape(img_size, pixel_format="rgb"):
    """frame_shape for CAMERA frames: a 'bgr' / 'rgba' / 'bgra' camera frame is at least 2 pixels wide (the undistortion fetches the
    two taps of a row as one window); a sink may be narrower."""
    tail = frame_shape(img_size, pixel_format)
    if pixel_format in RGB_FAMILY and int(img_size[0]) < 2:
        raise ValueError("%r camera frames need a width of at least 2, got %dx%d" % (pixel_format, int(img_size[0]), int(img_size[1])))
    return tail


_lib = None


def build(force=False):
    """Compile the shared library in-tree with hipcc for gfx950 (csrc/Makefile)."""
    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", csrc, "-s", "-j8"] + (["-B"] if force else [])
    subprocess.check_call(cmd)
    return LIB_PATH


def load():
    """dlopen the library and bind every declared symbol.  Raises NativeError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  lane_tracker_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and this table ever diverge
        fn.restype = res
        fn.argtypes = args
    if lib.lt_abi_version() != ABI_VERSION:
        raise NativeError("ABI version mismatch between _native.py and liblane_tracker_amd.so")
    _lib = lib
    return lib


def exported_symbols():
    return list(_SIGNATURES)


def _check(rc):
    if rc != 0:
        msg = load().lt_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(msg)
        raise NativeError(f"lane_tracker_amd error {rc}: {msg}")


class _PinnedPool:
    """Page-locked host blocks behind NumPy arrays (lt_host_alloc).  An array handed out keeps its block until
    the array and every view of it are gone; the block then goes back to the pool (or to the driver once the pool
    holds enough of that size).  Beyond `limit` bytes outstanding, or when the allocation fails, callers get a
    plain NumPy array -- slower copies, same results."""

    def __init__(self, limit=8 << 30, keep_per_size=4):
        self.limit, self.keep = limit, keep_per_size
        self.free, self.outstanding, self.kinds = {}, 0, {}

    def empty(self, shape, dtype=np.uint8):
        nbytes = math.prod(shape) * np.dtype(dtype).itemsize
        if nbytes == 0 or self.outstanding + nbytes > self.limit:
            return np.empty(shape, dtype)
        blocks = self.free.get(nbytes)
        if blocks:
            ptr = blocks.pop()
        else:
            out = C.c_void_p()
            if load().lt_host_alloc(nbytes, C.byref(out)) != 0 or not out.value:
                return np.empty(shape, dtype)
            ptr = out.value
        kind = self.kinds.get(nbytes)
        if kind is None:
            kind = self.kinds[nbytes] = C.c_uint8 * nbytes
        buf = kind.from_address(ptr)
        self.outstanding += nbytes
        fin = weakref.finalize(buf, self._release, nbytes, ptr)
        fin.atexit = False                       # at interpreter exit the driver reclaims everything
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def _release(self, nbytes, ptr):
        self.outstanding -= nbytes
        blocks = self.free.setdefault(nbytes, [])
        if len(blocks) < self.keep:
            blocks.append(ptr)
        else:
            load().lt_host_free(ptr)


_pinned = _PinnedPool()


class _FramePool:
    """Ordinary (pageable) host blocks behind the NumPy arrays a window of annotated frames is handed out in.  A fresh
    anonymous mapping costs a page fault -- and a cleared page -- per 4 KB (2 MB with transparent huge pages) at first touch:
    0.7 GB per window of 256 1280x720 frames, 40-50 ms spread over the copy threads, as much as the rest of the window
    takes.  So the blocks are kept: an array handed out keeps its block until the array and every view of it are gone, then the
    block waits here for the next window of that size.  At most `keep` blocks per size and `limit` bytes idle are kept
    (`frames_pool_limit` changes them; `frames_trim()` gives the idle blocks back -- `LaneTracker.close()` calls it when the last
    tracker of the process closes).  Returned frames are VIEWS of one window-sized block: keeping one frame keeps its window's
    block alive (copy the frame to let the window go)."""

    def __init__(self, limit=8 << 30, keep_per_size=5):
        self.limit, self.keep = limit, keep_per_size
        self.free, self.idle_bytes = {}, 0

    def empty(self, shape, dtype=np.uint8):
        import mmap
        nbytes = math.prod(shape) * np.dtype(dtype).itemsize
        if nbytes < (1 << 20):
            return np.empty(shape, dtype)
        blocks = self.free.get(nbytes)
        if blocks:
            mm = blocks.pop()
            self.idle_bytes -= nbytes
        else:
            try:
                mm = mmap.mmap(-1, nbytes)
                if hasattr(mmap, "MADV_HUGEPAGE"):
                    try:
                        mm.madvise(mmap.MADV_HUGEPAGE)
                    except OSError:
                        pass
            except (OSError, ValueError):
                return np.empty(shape, dtype)
        buf = (C.c_uint8 * nbytes).from_buffer(mm)
        fin = weakref.finalize(buf, self._release, nbytes, mm)
        fin.atexit = False
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def _release(self, nbytes, mm):
        blocks = self.free.setdefault(nbytes, [])
        if len(blocks) < self.keep and self.idle_bytes + nbytes <= self.limit:
            blocks.append(mm)
            self.idle_bytes += nbytes
        # else: the mapping goes with its last reference

    def trim(self):
        self.free, self.idle_bytes = {}, 0

    def prefault(self, shape, count, dtype=np.uint8):
        """Make sure `count` blocks for arrays of this shape wait in the pool with every page touched (by the library's copy
        threads): a stream's first windows then find their output memory in place.  First touch of fresh memory runs at about
        10 GB/s on the GPU boxes whatever the thread count (0.7 GB per window of 256 1280x720 frames: 70 ms)."""
        nbytes = math.prod(shape) * np.dtype(dtype).itemsize
        fresh = [self.empty(shape, dtype) for _ in range(min(count, self.keep))]      # (blocks that wait already come first: touching them again costs nothing)
        if fresh and nbytes >= (1 << 20):
            g = host_copy_group()
            lib = load()
            for a in fresh:
                rc = lib.lt_host_touch_async_group(g, a.ctypes.data, nbytes)
                if rc:
                    _check(rc)
            host_copy_group_release(g)
        del fresh                        # (back into the pool, touched)


_frames = _FramePool()


def frames_trim():
    """Give the idle blocks of the frame pool back to the system (blocks behind arrays still alive stay with their arrays)."""
    _frames.trim()


def frames_pool_limit(idle_bytes=None, keep_per_size=None):
    """Limits of the frame pool: at most `idle_bytes` of idle blocks and `keep_per_size` idle blocks per window size (defaults:
    8 GB, 5 -- a stream keeps four windows in flight).  -> (idle_bytes, keep_per_size) in force."""
    if idle_bytes is not None:
        _frames.limit = int(idle_bytes)
    if keep_per_size is not None:
        _frames.keep = int(keep_per_size)
    return _frames.limit, _frames.keep


def frames_prefault(shape, count):
    """`count` touched blocks for arrays of `shape` in the frame pool (see _FramePool.prefault)."""
    _frames.prefault(shape, count)


def frames_empty(shape, dtype=np.uint8):
    """An uninitialised array in ordinary host memory out of a pool of kept blocks (no first-touch page faults after the first
    windows of a stream): what process_batch / process_stream return their annotated frames in."""
    return _frames.empty(shape, dtype)


def device_cache_trim(keep_bytes=0):
    """Hand the device memory closed contexts left in the library's cache back to the driver (all of it beyond keep_bytes)."""
    _check(load().lt_device_cache_trim(int(keep_bytes)))


def host_copy_group():
    """A fresh completion group of the library's host copy threads (lt_host_copy_group_create)."""
    g = C.c_int(0)
    _check(load().lt_host_copy_group_create(C.byref(g)))
    return g.value


def host_copy_group_release(group):
    """Wait for the group's copies and forget it (lt_host_copy_group_destroy)."""
    _check(load().lt_host_copy_group_destroy(int(group)))


def text_bytes(lines_per_frame, line_len=40):
    """[[str, ...], ...] -> (bytes, n_lines): every frame's lines NUL-padded to line_len, frames padded to the longest list."""
    nl = max((len(l) for l in lines_per_frame), default=0)
    blank = b"\0" * line_len
    return b"".join(b"".join(t.encode("ascii", "replace")[:line_len].ljust(line_len, b"\0") for t in lines) + blank * (nl - len(lines))
                    for lines in lines_per_frame), nl


def text_blend(frames, font, text, n_lines, line_len=40, origin=(20, 8), step=35):
    """The text lines of `frames` (n, H, W, 3) u8 drawn in place on the calling thread (lt_text_blend_host: lt_overlay_text's
    arithmetic on the host).  font = (atlas (g, gh, gw) u8, advance (g,) u8, first_char); text = n * n_lines * line_len bytes."""
    f = _font_args.get(id(font))
    if f is None or f[0] is not font:                 # (addresses and sizes of a font, once: .ctypes.data costs a microsecond a time)
        atlas, advance, first_char = font
        f = _font_args[id(font)] = (font, atlas.ctypes.data, advance.ctypes.data, int(first_char), atlas.shape[0], atlas.shape[2], atlas.shape[1])
    n, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    rc = (_lib or load()).lt_text_blend_host(frames.ctypes.data, H * W * 3, n, H, W, f[1], f[2], f[3], f[4], f[5], f[6], text, n_lines, line_len,
                                 int(origin[0]), int(origin[1]), int(step))
    if rc:
        _check(rc)


_font_args = {}


def host_text_async(group, dst, src, rows, font, text, n_lines, line_len=40, origin=(20, 8), step=35):
    """On the library's copy threads, in `group`: the two runs of rows `rows` = (a0, a1, b0, b1) (or one run (a0, a1)) of every frame
    of `src` into `dst` (both (n, H, W, 3) u8, C-contiguous), then that frame's text lines drawn over them
    (lt_host_text_async_group).  font None / n_lines 0: only the rows."""
    n, H, W = dst.shape[0], dst.shape[1], dst.shape[2]
    if font is None or not n_lines:
        atlas = advance = None
        first_char = g = gw = gh = 0
        text, n_lines = None, 0
    else:
        atlas, advance, first_char = font
        g, gh, gw = atlas.shape
    r4 = np.array((list(rows) + [H, H])[:4] if len(rows) == 2 else list(rows), np.int32)
    _check(load().lt_host_text_async_group(int(group), dst.ctypes.data, H * W * 3, src.ctypes.data, H * W * 3, n, r4.ctypes.data, H, W,
                                           None if atlas is None else atlas.ctypes.data, None if advance is None else advance.ctypes.data,
                                           int(first_char), int(g), int(gw), int(gh), text, int(n_lines), int(line_len), int(origin[0]),
                                           int(origin[1]), int(step)))


def host_text_now(group, frame, font, text, n_lines, line_len=40, origin=(20, 8), step=35):
    """The text lines of ONE frame `frame` (1, H, W, 3) u8, drawn before the call returns and behind the copies of `group`
    (lt_host_text_now_group): the wait for the rows under the text and the drawing in one call."""
    f = _font_args.get(id(font))
    if f is None or f[0] is not font:
        atlas, advance, first_char = font
        f = _font_args[id(font)] = (font, atlas.ctypes.data, advance.ctypes.data, int(first_char), atlas.shape[0], atlas.shape[2], atlas.shape[1])
    rc = (_lib or load()).lt_host_text_now_group(group, frame.ctypes.data, frame.shape[1], frame.shape[2], f[1], f[2], f[3], f[4], f[5], f[6], text,
                                                 n_lines, line_len, origin[0], origin[1], step)
    if rc:
        _check(rc)


def host_copy_stats():
    """{'busy_s', 'bytes', 'pieces', 'threads'} of the library's copy threads since the process started (lt_host_copy_stats)."""
    b, y, p, t = C.c_double(), C.c_double(), C.c_longlong(), C.c_int()
    _check(load().lt_host_copy_stats(C.byref(b), C.byref(y), C.byref(p), C.byref(t)))
    return {"busy_s": b.value, "bytes": y.value, "pieces": p.value, "threads": t.value}


def device_cache_stats():
    """{'kept_bytes', 'live_bytes', 'limit_bytes', 'kept_blocks'} of the library's device-memory cache (lt_device_cache_stats)."""
    k, l, m, n = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
    _check(load().lt_device_cache_stats(C.byref(k), C.byref(l), C.byref(m), C.byref(n)))
    return {"kept_bytes": k.value, "live_bytes": l.value, "limit_bytes": m.value, "kept_blocks": n.value}


def host_memory_stats():
    """{'staging_bytes', 'queued_pieces', 'pending_pieces'}: page-locked staging the library holds, and the copy threads' backlog."""
    v = [C.c_size_t() for _ in range(3)]
    _check(load().lt_host_memory_stats(*[C.byref(x) for x in v]))
    return dict(zip(("staging_bytes", "queued_pieces", "pending_pieces"), (int(x.value) for x in v)))


def device_cache_counters():
    """{'hits', 'misses', 'evicted_blocks', 'evicted_bytes'} of the device-memory cache since the process started."""
    v = [C.c_ulonglong() for _ in range(4)]
    _check(load().lt_device_cache_counters(*[C.byref(x) for x in v]))
    return dict(zip(("hits", "misses", "evicted_blocks", "evicted_bytes"), (int(x.value) for x in v)))


def pinned_empty(shape, dtype=np.uint8):
    """An uninitialised array in page-locked host memory (falls back to np.empty)."""
    return _pinned.empty(shape, dtype)


def _u8(a, shape_tail=None):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a


def filter_params(filter_type="bilateral", ksize_r=15, C_r=8, ksize_b=35, C_b=5, mask_noise=False,
                  noise_thresh=140, ksize_noise=65, C_noise=10):
    ft = {"bilateral": 0, "neighborhood": 1}.get(filter_type, 2)   # 2 -> ValueError from the library (:220)
    return FilterParams(ft, int(ksize_r), int(C_r), int(ksize_b), int(C_b), int(bool(mask_noise)),
                        int(noise_thresh), int(ksize_noise), int(C_noise))


def search_params(window_width=30, window_height=40, search_range=20, mu=0.1, no_success_limit=8,
                  start_slice=0.25, ignore_sides=360, ignore_bottom=30, bandwidth=25, partial=1.0):
    return SearchParams(int(window_width), int(window_height), int(search_range), int(no_success_limit),
                        int(ignore_sides), int(ignore_bottom), int(bandwidth), 0, float(mu), float(start_slice),
                        float(partial))


def make_calib(img_size, warped_size, cam_matrix, dist_coeffs, M):
    cal = Calib()
    cal.img_w, cal.img_h = int(img_size[0]), int(img_size[1])
    cal.warp_w, cal.warp_h = int(warped_size[0]), int(warped_size[1])
    cal.cam_matrix[:] = [float(v) for v in np.asarray(cam_matrix, np.float64).reshape(9)]
    d = np.asarray(dist_coeffs, np.float64).reshape(-1)
    cal.dist_coeffs[:] = [float(v) for v in (list(d[:5]) + [0.0] * 5)[:5]]
    cal.M[:] = [float(v) for v in np.asarray(M, np.float64).reshape(9)]
    return cal


def calib_tables(cal):
    """The host-built calibration tables of a `Calib` (no GPU needed): dict with the warp map, the source-row
    window, the undistortion map of those rows, the Lab tables and the ellipse half-widths."""
    lib = load()
    r0, r1 = C.c_int(0), C.c_int(0)
    _check(lib.lt_calib_source_rows(C.byref(cal), C.byref(r0), C.byref(r1)))
    wxy = np.empty((cal.warp_h, cal.warp_w, 2), np.int16)
    wfr = np.empty((cal.warp_h, cal.warp_w), np.uint16)
    _check(lib.lt_calib_warp_table(C.byref(cal), wxy.ctypes.data, wfr.ctypes.data))
    uxy = np.empty((r1.value - r0.value, cal.img_w, 2), np.int16)
    ufr = np.empty((r1.value - r0.value, cal.img_w), np.uint16)
    _check(lib.lt_calib_undistort_table(C.byref(cal), r0.value, r1.value, uxy.ctypes.data, ufr.ctypes.data))
    gamma, cbrt, coef = np.empty(256, np.uint16), np.empty(3072, np.uint16), np.empty(9, np.int32)
    _check(lib.lt_calib_lab_tables(gamma.ctypes.data, cbrt.ctypes.data, coef.ctypes.data))
    ell = {}
    for k in (5, 29, 55):
        dx, taps = np.empty(k, np.int32), C.c_int(0)
        _check(lib.lt_calib_ellipse(k, dx.ctypes.data, C.byref(taps)))
        ell[k] = (dx, taps.value)
    return dict(source_rows=(r0.value, r1.value), warp_xy=wxy, warp_frac=wfr, und_xy=uxy, und_frac=ufr, gamma=gamma,
                cbrt=cbrt, lab_coeffs=coef, ellipse=ell)


def pack_polygons(polygons):
    """[(left_y, left_x, right_y, right_x), ...] -> (left counts, right counts, left (y, x) pairs, right (y, x) pairs), the
    form lt_overlay_run takes."""
    ln = np.array([len(p[0]) for p in polygons], np.int32)
    rn = np.array([len(p[2]) for p in polygons], np.int32)

    def pairs(ys, xs, counts):
        out = np.empty((int(counts.sum()), 2), np.int32)
        at = 0
        for y, x, m in zip(ys, xs, counts):
            out[at:at + m, 0] = y
            out[at:at + m, 1] = x
            at += m
        return out
    return ln, rn, pairs([p[0] for p in polygons], [p[1] for p in polygons], ln), pairs([p[2] for p in polygons], [p[3] for p in polygons], rn)


def split_panes_size(img_size, warped_size):
    """(scaled_w, scaled_h, second_x) of triple_split_view (reference :781-787) for a camera / bird's-eye size pair (width, height):
    the panes' size and the second pane's column.  Host-only (lt_calib_split_panes_size)."""
    cal = Calib()
    cal.img_w, cal.img_h, cal.warp_w, cal.warp_h = int(img_size[0]), int(img_size[1]), int(warped_size[0]), int(warped_size[1])
    a, b, c_ = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(load().lt_calib_split_panes_size(C.byref(cal), C.byref(a), C.byref(b), C.byref(c_)))
    return a.value, b.value, c_.value


def poly_points(warped_size, coeffs, ploty, ploty2):
    """get_poly_points (reference :511-528) for many pairs of parabolas at once, packed for overlay_run_packed: coeffs (n, 6)
    = left a, b, c, right a, b, c; ploty / ploty2 as LaneTracker._plot_rows gives them.  Host-only (lt_poly_points)."""
    lib = load()
    coeffs = np.ascontiguousarray(coeffs, np.float64).reshape(-1, 6)
    ploty, ploty2 = np.ascontiguousarray(ploty, np.float64), np.ascontiguousarray(ploty2, np.float64)
    n, rows = coeffs.shape[0], ploty.shape[0]
    ln, rn = np.empty(n, np.int32), np.empty(n, np.int32)
    lyx, ryx = np.empty((n * rows, 2), np.int32), np.empty((n * rows, 2), np.int32)
    _check(lib.lt_poly_points(int(warped_size[0]), int(warped_size[1]), coeffs.ctypes.data, n, ploty.ctypes.data, ploty2.ctypes.data,
                              rows, ln.ctypes.data, rn.ctypes.data, lyx.ctypes.data, ryx.ctypes.data))
    return ln, rn, lyx[:int(ln.sum())], ryx[:int(rn.sum())]


class Context:
    """One device context = one HIP stream + calibration tables + `capacity` frame slots in HBM."""

    def __init__(self, img_size, warped_size, cam_matrix, dist_coeffs, M, device=0, capacity=1):
        self._h = None
        lib = load()
        cal = make_calib(img_size, warped_size, cam_matrix, dist_coeffs, M)
        h = _P()
        _check(lib.lt_create(C.byref(cal), int(device), C.byref(h)))
        self._h = h
        self.lib = lib
        self.img_w, self.img_h, self.warp_w, self.warp_h = cal.img_w, cal.img_h, cal.warp_w, cal.warp_h
        self._pixel_format = "rgb"                       # the camera frames' pixel format (set_input_format)
        self._frame_tail = (cal.img_h, cal.img_w, 3)     # shape of one camera frame as the uploads take it (set_input_format, set_input_size)
        self._input_size = None                          # (width, height) of the frames the uploads take when it is not the calibration's
        self.reserve(capacity)

    def close(self):
        if self._h is not None:
            self.lib.lt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- bookkeeping
    def reserve(self, capacity):
        _check(self.lib.lt_reserve(self._h, int(capacity)))
        self.capacity = max(getattr(self, "capacity", 0), int(capacity))

    def info(self):
        i = Info()
        _check(self.lib.lt_get_info(self._h, C.byref(i)))
        return i

    def sync(self):
        _check(self.lib.lt_sync(self._h))

    def set_streams(self, n):
        """Spread the slots over n HIP streams (slices of the capacity overlap each other's stages)."""
        _check(self.lib.lt_set_streams(self._h, int(n)))

    # -- data movement
    def set_input_format(self, pixel_format="rgb", yuv_matrix="bt601"):
        """The pixel format of the camera frames this context takes, once, before its first upload: 'rgb' (the default), or
        'nv12' / 'i420' -- frames of shape (H * 3 // 2, W) as OpenCV holds them -- or packed 4:2:2, 'yuy2' / 'uyvy' -- frames of shape
        (H, W, 2) -- converted on the device with `yuv_matrix` ('bt601', 'bt709', or five integers); or another member of the RGB
        family, 'bgr' -- (H, W, 3), OpenCV's order -- / 'rgba' / 'bgra' -- (H, W, 4), alpha not read --, a channel permutation
        (`yuv_matrix` is ignored as for 'rgb'); or 8-bit raw Bayer, 'bayer_rggb' / 'bayer_grbg' / 'bayer_gbrg' / 'bayer_bggr' -- frames of
        shape (H, W), H and W even and at least 4, demosaiced on the device (`yuv_matrix` ignored).  Every upload method then takes
        such frames."""
        layout = pixel_format_id(pixel_format)
        tail = input_frame_shape((self.img_w, self.img_h), pixel_format)
        k = yuv_coeffs(yuv_matrix) if is_yuv(layout) else None
        if layout and self._input_size is not None:
            raise ValueError("a context with an input size takes RGB frames only: %r frames are not resized" % (pixel_format,))
        _check(self.lib.lt_set_input_format(self._h, layout, None if k is None else k.ctypes.data))
        self._frame_tail = tail
        self._pixel_format = pixel_format

    def set_input_size(self, size):
        """Frames of another size: the uploads take RGB frames (Hi, Wi, 3) of `size` = (Wi, Hi) and resize them on the device to the
        calibration's size -- `cv2.resize(frame, img_size)`, INTER_LINEAR, bit for bit (lt_set_input_size).  Once, before the first
        upload, RGB contexts only; None or the calibration's own size clears the setting."""
        w, h = (self.img_w, self.img_h) if size is None else (int(size[0]), int(size[1]))
        _check(self.lib.lt_set_input_size(self._h, w, h))
        plain = (w, h) == (self.img_w, self.img_h)
        self._input_size = None if plain else (w, h)
        self._frame_tail = (h, w, 3)

    def input_size(self):
        """-> (width, height) of the frames the uploads take (lt_get_input_size)."""
        w, h = C.c_int(0), C.c_int(0)
        _check(self.lib.lt_get_input_size(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def input_rows(self):
        """Rows [row0, row1) of a frame of the input size that upload_frame_rows moves (lt_get_input_rows): source_rows() without an
        input size."""
        a, b = C.c_int(0), C.c_int(0)
        _check(self.lib.lt_get_input_rows(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def input_format(self):
        """-> (pixel format name, the five conversion coefficients)."""
        layout, k = C.c_int(0), np.zeros(5, np.int32)
        _check(self.lib.lt_get_input_format(self._h, C.byref(layout), k.ctypes.data))
        return format_name(layout.value), tuple(int(v) for v in k)

    def _frames(self, frames):
        """`frames` as the C-contiguous block (n,) + one frame's shape -- u8; uint16 for 10- / 12-bit raw Bayer --; ValueError for frames
        of another shape."""
        f = frames_array(frames, self._pixel_format)
        tail = self._frame_tail
        if f.shape[-len(tail):] != tail or f.ndim > len(tail) + 1:
            if self._pixel_format == "rgb" and self._input_size is None:
                return f.reshape((-1,) + tail)           # (RGB: anything of the right size, as ever)
            raise ValueError("expected camera frames of shape %r, got %r" % (tail, f.shape))
        return f.reshape((-1,) + tail)

    def yuv_to_rgb(self, frame, layout="nv12", matrix="bt601"):
        """One 4:2:0 frame (H * 3 // 2, W), or one packed 4:2:2 frame (H, W, 2), -> RGB (H, W, 3), on the device (lt_yuv_to_rgb)."""
        a = _u8(frame)
        if not is_yuv(pixel_format_id(layout)):
            raise ValueError("layout must be 'nv12', 'i420', 'yuy2' or 'uyvy'")
        if layout in PACKED_422:
            if a.ndim != 3 or a.shape[2] != 2 or a.shape[1] % 2 or a.shape[1] < 4 or a.shape[0] < 1:
                raise ValueError("a 4:2:2 frame is an array of shape (H, W, 2) with W even and at least 4, got %r" % (a.shape,))
            out = np.empty((a.shape[0], a.shape[1], 3), np.uint8)
            k = yuv_coeffs(matrix)
            _check(self.lib.lt_yuv_to_rgb(self._h, a.ctypes.data, a.shape[0], a.shape[1], pixel_format_id(layout), k.ctypes.data, out.ctypes.data))
            return out
        if a.ndim != 2 or a.shape[0] % 3 or a.shape[1] % 2 or (a.shape[0] // 3 * 2) % 2:
            raise ValueError("a 4:2:0 frame is a 2-D array of shape (H * 3 // 2, W) with H and W even, got %r" % (a.shape,))
        h, w = a.shape[0] // 3 * 2, a.shape[1]
        out = np.empty((h, w, 3), np.uint8)
        k = yuv_coeffs(matrix)
        _check(self.lib.lt_yuv_to_rgb(self._h, a.ctypes.data, h, w, pixel_format_id(layout), k.ctypes.data, out.ctypes.data))
        return out

    def set_raw_lut(self, lut, raw_set=0):
        """The raw table of a raw Bayer context -- u8 (4, 256), `utils.raw_lut` -- or None for none (lt_set_raw_lut): every sample is
        looked up in the row of its colour phase before the demosaic, in the undistortion and in the row conversion launched from now
        on.  Waits for the context's outstanding work: a set-up or occasional call, not a per-frame one.  A 10- / 12-bit context:
        u8 (4, 2**bits), None for the default `utils.raw_lut(bits=..)` (lt_set_raw_lut_wide).  `raw_set`: the raw set of the context
        that takes it (`add_raw_set`; lt_set_raw_lut_of), 0: the context's own."""
        a = checked_raw_lut(lut, self._pixel_format)
        if raw_set:
            _check(self.lib.lt_set_raw_lut_of(self._h, int(raw_set), None if a is None else a.ctypes.data, 1 << raw_bits(self._pixel_format)))
            return
        if self._pixel_format in BAYER_DEEP_FORMATS:
            _check(self.lib.lt_set_raw_lut_wide(self._h, None if a is None else a.ctypes.data, 1 << raw_bits(self._pixel_format)))
            return
        _check(self.lib.lt_set_raw_lut(self._h, None if a is None else a.ctypes.data))

    def raw_lut(self, raw_set=0):
        """-> the raw table, u8 (4, 256), or None (lt_get_raw_lut); a 10- / 12-bit context: the table in effect, u8 (4, 2**bits)
        (lt_get_raw_lut_wide).  `raw_set`: of that raw set (lt_get_raw_lut_of)."""
        if raw_set:
            n = 1 << raw_bits(self._pixel_format)
            out, is_set = np.zeros((4, max(n, 1)), np.uint8), C.c_int(0)
            _check(self.lib.lt_get_raw_lut_of(self._h, int(raw_set), out.ctypes.data, n, C.byref(is_set)))
            return out if is_set.value else None
        if self._pixel_format in BAYER_DEEP_FORMATS:
            n = 1 << raw_bits(self._pixel_format)
            out = np.zeros((4, n), np.uint8)
            _check(self.lib.lt_get_raw_lut_wide(self._h, out.ctypes.data, n))
            return out
        out, is_set = np.zeros((4, 256), np.uint8), C.c_int(0)
        _check(self.lib.lt_get_raw_lut(self._h, out.ctypes.data, C.byref(is_set)))
        return out if is_set.value else None

    def set_raw_color(self, ccm=None, curve=None, enable=True, raw_set=0):
        """The colour stage of a raw Bayer context (lt_set_raw_color): `ccm` int16 (3, 3) in Q10 (`utils.raw_ccm`; None: the identity)
        and `curve` u8 (256,) (`utils.raw_curve`; None: the identity) on every demosaiced pixel, in the undistortion and in the row
        conversion launched from now on; enable=False removes it.  Waits for the context's outstanding work: a set-up or occasional
        call, not a per-frame one."""
        m, t = checked_raw_color(ccm, curve, self._pixel_format)
        args = (None if m is None else m.ctypes.data, None if t is None else t.ctypes.data, 1 if enable else 0)
        if raw_set:                          # of that raw set (lt_set_raw_color_of)
            _check(self.lib.lt_set_raw_color_of(self._h, int(raw_set), *args))
            return
        _check(self.lib.lt_set_raw_color(self._h, *args))

    def get_raw_color(self, raw_set=0):
        """-> (ccm int16 (3, 3), curve u8 (256,)) of the colour stage, or None without one (lt_get_raw_color; `raw_set`: lt_get_raw_color_of)."""
        m, t, is_set = np.zeros((3, 3), np.int16), np.zeros(256, np.uint8), C.c_int(0)
        if raw_set:
            _check(self.lib.lt_get_raw_color_of(self._h, int(raw_set), m.ctypes.data, t.ctypes.data, C.byref(is_set)))
            return (m, t) if is_set.value else None
        _check(self.lib.lt_get_raw_color(self._h, m.ctypes.data, t.ctypes.data, C.byref(is_set)))
        return (m, t) if is_set.value else None

    def set_raw_shading(self, shading, raw_set=0):
        """The lens-shading map of a raw Bayer context (lt_set_raw_shading): `shading` a `utils.RawShading` -- every sample corrected by
        the gain of its position before the raw table, in the undistortion and in the row conversion launched from now on -- or None,
        which removes it.  Waits for the context's outstanding work: a set-up or occasional call, not a per-frame one."""
        s = checked_raw_shading(shading, self._pixel_format)
        args = (None, 0, 0, None, 0) if s is None else (s.mesh.ctypes.data, s.mesh.shape[2], s.mesh.shape[1], s.black.ctypes.data, 1)
        if raw_set:                          # of that raw set (lt_set_raw_shading_of)
            _check(self.lib.lt_set_raw_shading_of(self._h, int(raw_set), *args))
            return
        _check(self.lib.lt_set_raw_shading(self._h, *args))

    def get_raw_shading(self, raw_set=0):
        """-> the utils.RawShading of the context, or None without one (lt_get_raw_shading; `raw_set`: lt_get_raw_shading_of)."""
        from .utils import RawShading
        get = (lambda *a: self.lib.lt_get_raw_shading_of(self._h, int(raw_set), *a)) if raw_set else (lambda *a: self.lib.lt_get_raw_shading(self._h, *a))
        mw, mh, is_set = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(get(None, C.byref(mw), C.byref(mh), None, C.byref(is_set)))
        if not is_set.value:
            return None
        mesh, black = np.zeros((4, mh.value, mw.value), np.uint16), np.zeros(4, np.int32)
        _check(get(mesh.ctypes.data, None, None, black.ctypes.data, None))
        return RawShading(mesh, black)

    def raw_shading_plane(self, raw_set=0):
        """-> the gain plane the device expanded the context's shading mesh into, uint16 (H, W) (lt_get_raw_shading_plane; `raw_set`:
        that set's, lt_get_raw_shading_plane_of)."""
        out = np.empty((self.img_h, self.img_w), np.uint16)
        if raw_set:
            _check(self.lib.lt_get_raw_shading_plane_of(self._h, int(raw_set), out.ctypes.data))
            return out
        _check(self.lib.lt_get_raw_shading_plane(self._h, out.ctypes.data))
        return out

    # -- raw sets: cameras of different raw tables, colour stages and shading maps in one context, one set per slot
    def add_raw_set(self):
        """A further raw set of the context, a copy of set 0's table, colour stage and shading map as they are now (lt_add_raw_set);
        returns its id.  The setters and getters above take it as `raw_set`."""
        i = C.c_int(0)
        _check(self.lib.lt_add_raw_set(self._h, C.byref(i)))
        return i.value

    def raw_set_count(self):
        n = C.c_int(0)
        _check(self.lib.lt_raw_set_count(self._h, C.byref(n)))
        return n.value

    def set_slot_raw_sets(self, ids, first=0):
        """Slot first + i takes raw set ids[i] (lt_set_slot_raw_sets)."""
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        _check(self.lib.lt_set_slot_raw_sets(self._h, int(first), a.shape[0], a.ctypes.data if a.shape[0] else None))

    def slot_raw_sets(self, n=None, first=0):
        """The raw sets of slots first, first + 1, ... (n of them; None: up to the capacity)."""
        n = self.capacity - first if n is None else int(n)
        a = np.zeros(max(n, 0), np.int32)
        _check(self.lib.lt_get_slot_raw_sets(self._h, int(first), a.shape[0], a.ctypes.data if a.shape[0] else None))
        return a

    def last_raw_walk_form(self):
        """Which raw walks the front end of the last mask_run launched: 0 none, 1 the one-set forms, 2 the set-per-slot forms; -1: no run yet."""
        return int(self.lib.lt_last_raw_walk_form(self._h))

    def raw_stats(self, n, first=0, grid=(8, 8), rows=None, cols=None, lo=None, hi=None):
        """Statistics of the raw Bayer frames slots first .. first + n hold -- the attached surfaces where a slot has them, what was uploaded
        otherwise --, of the samples as they enter the raw table, behind the context's shading map where it has one (lt_raw_stats): what
        `utils.raw_stats` defines, bit for bit, as a `utils.RawStats` with a leading frame axis.  rows=None: the rows every upload brings
        (`input_rows()`, rounded inward to even); other rows need whole frames in the slots (upload_frames, attached frames).  Waits for the
        context's outstanding work: an occasional call, not a per-frame one.  The arguments are checked before any device call (ValueError)."""
        from .utils import RawStats
        n, first = int(n), int(first)
        if n < 0 or first < 0 or first + n > self.capacity:
            raise ValueError("slots [%d, %d) outside the context's capacity %d" % (first, first + n, self.capacity))
        p = checked_raw_stats(self._pixel_format, (self.img_w, self.img_h), self.input_rows(), grid, rows, cols, lo, hi)
        zones = (p.grid_h, p.grid_w)
        hist = np.zeros((n, 4, max(1 << raw_bits(self._pixel_format), 256)), np.uint32)
        count, total = np.zeros((n,) + zones, np.uint32), np.zeros((n,) + zones + (4,), np.uint64)
        rect = np.zeros(4, np.int32)
        _check(self.lib.lt_raw_stats(self._h, first, n, C.byref(p), hist.ctypes.data, count.ctypes.data, total.ctypes.data, rect.ctypes.data))
        return RawStats(hist, count, total, (int(rect[0]), int(rect[1])), (int(rect[2]), int(rect[3])))

    def raw_to_rgb_shaded(self, frame, pattern, shading, raw_lut=None, ccm=None, curve=None):
        """`raw_to_rgb_color` behind the shading map `shading` (lt_raw_to_rgb_shaded); without `ccm` and `curve`: no colour stage."""
        if pattern not in RAW_FORMATS:
            raise ValueError("pattern must be one of %s, got %r" % (", ".join(repr(n) for n in RAW_FORMATS), pattern))
        a = frames_array(frame, pattern)
        lut = checked_raw_lut(raw_lut, pattern)
        m, t = checked_raw_color(ccm, curve, pattern)
        s = checked_raw_shading(shading, pattern)
        if s is None:
            raise ValueError("raw_to_rgb_shaded takes a shading map (raw_to_rgb_color: the conversion without one)")
        h, w = raw_frame_size(a, pattern)
        out = np.empty((h, w, 3), np.uint8)
        _check(self.lib.lt_raw_to_rgb_shaded(self._h, a.ctypes.data, h, w, pixel_format_id(pattern),
                                             None if lut is None else lut.ctypes.data, 1 << raw_bits(pattern),
                                             None if m is None else m.ctypes.data, None if t is None else t.ctypes.data,
                                             s.mesh.ctypes.data, s.mesh.shape[2], s.mesh.shape[1], s.black.ctypes.data, out.ctypes.data))
        return out

    def raw_to_rgb_color(self, frame, pattern, raw_lut=None, ccm=None, curve=None):
        """One raw Bayer frame (H, W) in any of the twelve raw patterns -> RGB (H, W, 3) with the colour stage, on the device
        (lt_raw_to_rgb_color): looked up in `raw_lut` (None: none / the 10- / 12-bit default), demosaiced, matrix, curve."""
        if pattern not in RAW_FORMATS:
            raise ValueError("pattern must be one of %s, got %r" % (", ".join(repr(n) for n in RAW_FORMATS), pattern))
        a = frames_array(frame, pattern)
        lut = checked_raw_lut(raw_lut, pattern)
        m, t = checked_raw_color(ccm, curve, pattern)
        h, w = raw_frame_size(a, pattern)
        out = np.empty((h, w, 3), np.uint8)
        _check(self.lib.lt_raw_to_rgb_color(self._h, a.ctypes.data, h, w, pixel_format_id(pattern),
                                            None if lut is None else lut.ctypes.data, 1 << raw_bits(pattern),
                                            None if m is None else m.ctypes.data, None if t is None else t.ctypes.data, out.ctypes.data))
        return out

    def bayer_to_rgb(self, frame, pattern="bayer_rggb", raw_lut=None):
        """One 8-bit raw Bayer frame (H, W), H and W even and at least 4, -> RGB (H, W, 3): the bilinear demosaic, on the device
        (lt_bayer_to_rgb).  A 10- / 12-bit pattern: one uint16 frame, every sample looked up in `raw_lut` -- u8 (4, 2**bits), None: the
        default -- first (lt_raw16_to_rgb)."""
        if pattern in BAYER_PACKED_FORMATS:      # packed rows: the colour-stage converter with the identity stage is the table alone
            return self.raw_to_rgb_color(frame, pattern, raw_lut)
        if pattern in BAYER_WIDE_FORMATS:
            a = frames_array(frame, pattern)
            lut = checked_raw_lut(raw_lut, pattern)
            if a.ndim != 2 or a.shape[0] % 2 or a.shape[1] % 2 or a.shape[0] < 4 or a.shape[1] < 4:
                raise ValueError("a raw Bayer frame is a 2-D array of shape (H, W) with H and W even and at least 4, got %r" % (a.shape,))
            out = np.empty((a.shape[0], a.shape[1], 3), np.uint8)
            _check(self.lib.lt_raw16_to_rgb(self._h, a.ctypes.data, a.shape[0], a.shape[1], BAYER_WIDE_FORMATS[pattern],
                                            None if lut is None else lut.ctypes.data, out.ctypes.data))
            return out
        if raw_lut is not None:
            raise ValueError("bayer_to_rgb takes a raw_lut with the 10- and 12-bit patterns only (8-bit: utils.apply_raw_lut first)")
        a = _u8(frame)
        if pattern not in BAYER_FORMATS:
            raise ValueError("pattern must be one of %s, got %r" % (", ".join(repr(n) for n in BAYER_FORMATS), pattern))
        if a.ndim != 2 or a.shape[0] % 2 or a.shape[1] % 2 or a.shape[0] < 4 or a.shape[1] < 4:
            raise ValueError("a raw Bayer frame is a 2-D array of shape (H, W) with H and W even and at least 4, got %r" % (a.shape,))
        out = np.empty((a.shape[0], a.shape[1], 3), np.uint8)
        _check(self.lib.lt_bayer_to_rgb(self._h, a.ctypes.data, a.shape[0], a.shape[1], BAYER_FORMATS[pattern], out.ctypes.data))
        return out

    # -- calibration sets: cameras of different calibrations in one context, one per slot
    def add_calibration(self, cam_matrix, dist_coeffs, M):
        """A further calibration set of the context's image and bird's-eye sizes, before the first upload (lt_add_calibration);
        returns its id.  Set 0 is the calibration the context was created with."""
        cal = make_calib((self.img_w, self.img_h), (self.warp_w, self.warp_h), cam_matrix, dist_coeffs, M)
        i = C.c_int(0)
        _check(self.lib.lt_add_calibration(self._h, C.byref(cal), C.byref(i)))
        return i.value

    def calibration_count(self):
        n = C.c_int(0)
        _check(self.lib.lt_calibration_count(self._h, C.byref(n)))
        return n.value

    def set_slot_calibrations(self, ids, first=0):
        """Slot first + i takes calibration set ids[i] (lt_set_slot_calibrations)."""
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        _check(self.lib.lt_set_slot_calibrations(self._h, int(first), a.shape[0], a.ctypes.data if a.shape[0] else None))

    def slot_calibrations(self, n=None, first=0):
        """The calibration sets of slots first, first + 1, ... (n of them; None: up to the capacity)."""
        n = self.capacity - first if n is None else int(n)
        a = np.zeros(max(n, 0), np.int32)
        _check(self.lib.lt_get_slot_calibrations(self._h, int(first), n, a.ctypes.data if n > 0 else None))
        return a

    def source_rows(self):
        """Camera rows [row0, row1) the path reads."""
        a, b = C.c_int(0), C.c_int(0)
        _check(self.lib.lt_get_source_rows(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        """Like upload_frames, but only the camera rows the path reads cross the bus (not enough for the overlay).
        enqueue: no wait for the copy (lt_upload_frame_rows_enqueue) -- the array handed to the library is returned and must stay
        alive and unchanged until a call that waits for work launched over these slots afterwards (download_record, sync)."""
        f = self._frames(frames)
        if enqueue:
            _check(self.lib.lt_upload_frame_rows_enqueue(self._h, f.ctypes.data, first, f.shape[0]))
            return f
        _check(self.lib.lt_upload_frame_rows(self._h, f.ctypes.data, first, f.shape[0]))

    def upload_frame_rows_async(self, frames, first=0):
        """Stream-ordered upload_frame_rows (no host wait).  `frames` must be a C-contiguous u8 array that stays alive
        and unchanged until the next sync() -- use pinned_empty() for it; returns the array handed to the library."""
        f = np.asarray(frames)
        if f.dtype != frame_dtype(self._pixel_format) or not f.flags["C_CONTIGUOUS"]:
            raise ValueError("upload_frame_rows_async needs a C-contiguous %s array (no hidden copy may be made)" % frame_dtype(self._pixel_format))
        f = self._frames(f)
        _check(self.lib.lt_upload_frame_rows_async(self._h, f.ctypes.data, first, f.shape[0]))
        return f

    def upload_frame_rest(self, frames, first=0, rows=None):
        """The rows upload_frame_rows left out, on a copy stream beside the compute streams (for the overlay); with `rows` (the
        ADDRESS of four int32 {a0, a1, b0, b1}) only those of them inside the two runs -- what present_frame with the same runs
        reads.  Returns the array actually handed to the library: keep it alive until the next sync() / download."""
        f = self._frames(frames)
        if rows is None:
            _check(self.lib.lt_upload_frame_rest(self._h, f.ctypes.data, first, f.shape[0]))
        else:
            _check(self.lib.lt_upload_frame_rest_rows(self._h, f.ctypes.data, first, f.shape[0], rows))
        return f

    def attach_device_frames(self, frames, first=0):
        """The front end of slots first, first + 1, ... reads `frames` (a device.DeviceFrames) where they lie in device memory
        (lt_attach_device_frames); nothing is copied.  Returns `frames`: keep it -- and the memory it describes -- alive and
        unchanged until a call that waits for work launched over these slots afterwards (download_record, sync)."""
        if self._input_size is not None:
            raise ValueError("a context with an input size takes host frames only: frames in device memory are not resized")
        frames.check_for((self.img_w, self.img_h), self._pixel_format)
        frames.wait_for_producer()
        s = np.ascontiguousarray(frames.surfaces)
        _check(self.lib.lt_attach_device_frames(self._h, s.ctypes.data, first, s.shape[0]))
        return frames

    def device_frames_rest(self, n, first=0, rows=None):
        """The rows a shown frame needs, from the attached surfaces into the slots' RGB camera frames, on the device beside the mask
        chain (lt_device_frames_rest); `rows`: the ADDRESS of four int32 {a0, a1, b0, b1}, or None for the whole frame."""
        _check(self.lib.lt_device_frames_rest(self._h, first, int(n), rows))

    def _frame_list(self, frames):
        fs = [frames_array(f, self._pixel_format) for f in frames]
        for f in fs:
            if f.shape != self._frame_tail:
                raise ValueError("expected frames of shape %r, got %r" % (self._frame_tail, f.shape))
        ptrs = (C.c_void_p * max(len(fs), 1))(*[f.ctypes.data for f in fs])
        return fs, ptrs

    def upload_frame_rows_list(self, frames, first=0):
        """upload_frame_rows(enqueue=True) of separate frames (a sequence of (H, W, 3) arrays) into slots first, first + 1, ...
        (lt_upload_frame_rows_list).  Returns the arrays handed to the library: keep them alive as upload_frame_rows' result."""
        fs, ptrs = self._frame_list(frames)
        _check(self.lib.lt_upload_frame_rows_list(self._h, C.cast(ptrs, C.c_void_p), first, len(fs)))
        return fs

    def upload_frame_rest_list(self, frames, first=0):
        """upload_frame_rest of separate frames into slots first, first + 1, ... (lt_upload_frame_rest_list).  Returns the arrays
        handed to the library: keep them alive until the next sync() / download."""
        fs, ptrs = self._frame_list(frames)
        _check(self.lib.lt_upload_frame_rest_list(self._h, C.cast(ptrs, C.c_void_p), first, len(fs)))
        return fs

    def search_fit_list(self, items, sws=None, band=None):
        """The searches of a list of frames, each in its own slot and mode, in one launch (lt_search_fit_list).  `items`: an array
        of SEARCH_ITEM_DTYPE, or (slot, mode, prev_coeffs or None) tuples; sws / band: search_params() (None: the defaults)."""
        if not (isinstance(items, np.ndarray) and items.dtype == SEARCH_ITEM_DTYPE):
            lst = list(items)
            arr = np.zeros(len(lst), SEARCH_ITEM_DTYPE)
            for i, (slot, mode, prev) in enumerate(lst):
                arr[i]["slot"], arr[i]["mode"] = slot, mode
                if prev is not None:
                    arr[i]["prev_coeffs"] = np.asarray(prev, np.float64).reshape(6)
            items = arr
        items = np.ascontiguousarray(items)
        sws = sws or search_params()
        band = band or search_params()
        _check(self.lib.lt_search_fit_list(self._h, len(items), items.ctypes.data if len(items) else None, C.byref(sws), C.byref(band)))

    def upload_frames(self, frames, first=0):
        f = self._frames(frames)
        _check(self.lib.lt_upload_frames(self._h, f.ctypes.data, first, f.shape[0]))
        return f.shape[0]

    def upload_masks(self, masks, first=0):
        m = _u8(masks).reshape(-1, self.warp_h, self.warp_w)
        _check(self.lib.lt_upload_masks(self._h, m.ctypes.data, first, m.shape[0]))
        return m.shape[0]

    def upload_mask_bits(self, masks, first=0):
        """u8 or bool masks (n, warp_h, warp_w), a pixel set where != 0, uploaded as bit planes (lt_upload_mask_bits): the
        searches over these slots take the bit-plane kernels."""
        from .utils import pack_mask_bits
        m = np.asarray(masks).reshape(-1, self.warp_h, self.warp_w)
        bits = np.ascontiguousarray(pack_mask_bits(m))
        _check(self.lib.lt_upload_mask_bits(self._h, bits.ctypes.data, first, m.shape[0]))
        return m.shape[0]

    def upload_bev(self, bev, first=0):
        b = _u8(bev).reshape(-1, self.warp_h, self.warp_w, 3)
        _check(self.lib.lt_upload_bev(self._h, b.ctypes.data, first, b.shape[0]))
        return b.shape[0]

    def download_masks(self, n, first=0):
        out = np.empty((n, self.warp_h, self.warp_w), np.uint8)
        _check(self.lib.lt_download_masks(self._h, first, n, out.ctypes.data))
        return out

    def download_plane(self, plane, n, first=0):
        out = np.empty((n, self.warp_h, self.warp_w), np.uint8)
        _check(self.lib.lt_download_plane(self._h, plane, first, n, out.ctypes.data))
        return out

    def download_undistorted(self, n, first=0):
        i = self.info()
        out = np.empty((n, i.src_row1 - i.src_row0, self.img_w, 3), np.uint8)
        _check(self.lib.lt_download_undistorted(self._h, first, n, out.ctypes.data))
        return out

    # ---- presentation stage (draw_lane overlay, bird's-eye image) ----
    def overlay_configure(self, Minv, calibration=0):
        m = np.ascontiguousarray(Minv, np.float64).reshape(9)
        if calibration:
            _check(self.lib.lt_overlay_configure_set(self._h, int(calibration), m.ctypes.data))
        else:
            _check(self.lib.lt_overlay_configure(self._h, m.ctypes.data))

    def overlay_run(self, polygons, first=0, alpha=0.3, rows=None):
        """polygons: one (left_y, left_x, right_y, right_x) tuple per slot (empty arrays: plain copy); rows: None or the
        ADDRESS of four int32 {a0, a1, b0, b1} -- only these two runs of rows of every frame are drawn."""
        self.overlay_run_packed(*pack_polygons(polygons), first=first, alpha=alpha, rows=rows)

    def overlay_run_packed(self, ln, rn, lyx, ryx, first=0, alpha=0.3, rows=None):
        """The same with the polygons already packed (pack_polygons / poly_points): int32 counts per slot and the (y, x) pairs
        of all slots back to back."""
        ln, rn = np.ascontiguousarray(ln, np.int32), np.ascontiguousarray(rn, np.int32)
        lyx, ryx = np.ascontiguousarray(lyx, np.int32), np.ascontiguousarray(ryx, np.int32)
        if len(rn) != len(ln) or lyx.size != 2 * int(ln.sum()) or ryx.size != 2 * int(rn.sum()):
            raise ValueError("point lists do not match their counts")
        _check(self.lib.lt_overlay_run_rows(self._h, first, len(ln), ln.ctypes.data, rn.ctypes.data,
                                            lyx.ctypes.data if lyx.size else None, ryx.ctypes.data if ryx.size else None,
                                            float(alpha), rows))

    def overlay_run_strip_packed(self, ln, rn, lyx, ryx, first=0, alpha=0.3):
        """overlay_run_packed in strip mode (lt_overlay_run_strip): only the rows the lane can reach, packed per slot."""
        ln, rn = np.ascontiguousarray(ln, np.int32), np.ascontiguousarray(rn, np.int32)
        lyx, ryx = np.ascontiguousarray(lyx, np.int32), np.ascontiguousarray(ryx, np.int32)
        if len(rn) != len(ln) or lyx.size != 2 * int(ln.sum()) or ryx.size != 2 * int(rn.sum()):
            raise ValueError("point lists do not match their counts")
        _check(self.lib.lt_overlay_run_strip(self._h, first, len(ln), ln.ctypes.data, rn.ctypes.data,
                                             lyx.ctypes.data if lyx.size else None, ryx.ctypes.data if ryx.size else None, float(alpha)))

    def overlay_run_strip_coeffs(self, coeffs, draw, ploty, ploty2, first=0, alpha=0.3):
        """Strips from the lanes' averaged coefficients (lt_overlay_run_strip_coeffs): coeffs (n, 6) f64, draw (n,) u8 (0: no lane in
        that frame); plot points and polygon intervals are formed on the device.  -> False where that form does not exist."""
        coeffs = np.ascontiguousarray(coeffs, np.float64).reshape(-1, 6)
        draw = np.ascontiguousarray(draw, np.uint8)
        if len(draw) != len(coeffs):
            raise ValueError("one draw byte per frame")
        rc = self.lib.lt_overlay_run_strip_coeffs(self._h, first, len(coeffs), coeffs.ctypes.data, draw.ctypes.data, ploty.ctypes.data,
                                                  ploty2.ctypes.data, len(ploty), float(alpha))
        if rc == -5:
            return False
        if rc:
            _check(rc)
        return True

    def strip_download_async(self, out, first, group):
        """The strips of slots first .. first+len(out)-1 into rows overlay_rows() of the frames `out` (n, H, W, 3) u8, C-contiguous,
        ordinary memory; complete when the host-copy group `group` has been waited for (lt_strip_download_async)."""
        if out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] or out.shape[1:] != (self.img_h, self.img_w, 3):
            raise ValueError("strip_download_async needs a C-contiguous uint8 array (n, H, W, 3)")
        _check(self.lib.lt_strip_download_async(self._h, first, out.shape[0], out.ctypes.data, self.img_h * self.img_w * 3, int(group)))

    def warm(self, sws=None, band=None, annotate=0):
        """Set up now what the first searches / chains / overlays would set up on the way (lt_warm); annotate: 0 none, 1 whole
        annotated frames, 2 strips; + 4 the staging ring of search_viz_run, + 8 that of split_panes_run as well."""
        _check(self.lib.lt_warm(self._h, None if sws is None else C.byref(sws), None if band is None else C.byref(band), int(annotate)))

    def overlay_set_font(self, atlas, advance, first_char=32):
        """atlas: (n_glyphs, glyph_h, glyph_w) u8 alpha cells; advance: (n_glyphs,) u8."""
        atlas = np.ascontiguousarray(atlas, np.uint8)
        advance = np.ascontiguousarray(advance, np.uint8)
        _check(self.lib.lt_overlay_set_font(self._h, atlas.ctypes.data, advance.ctypes.data, int(first_char),
                                            atlas.shape[0], atlas.shape[2], atlas.shape[1]))

    def overlay_text(self, lines_per_slot, first=0, origin=(20, 8), step=35, line_len=40):
        """lines_per_slot: one list of strings per slot (ASCII)."""
        n = len(lines_per_slot)
        nl = max((len(l) for l in lines_per_slot), default=0)
        if n == 0 or nl == 0:
            return
        blank = b"\0" * line_len
        buf = b"".join(b"".join(t.encode("ascii", "replace")[:line_len].ljust(line_len, b"\0") for t in lines) + blank * (nl - len(lines))
                       for lines in lines_per_slot)
        _check(self.lib.lt_overlay_text(self._h, first, n, buf, nl, line_len, int(origin[0]), int(origin[1]), int(step)))

    def download_overlay(self, n, first=0):
        out = pinned_empty((n, self.img_h, self.img_w, 3))
        _check(self.lib.lt_download_overlay(self._h, first, n, out.ctypes.data))
        return out

    def download_overlay_async(self, out, first=0, rows=None):
        """Enqueue the copy of the annotated frames of slots first .. first+len(out)-1 into `out` (a C-contiguous u8 array
        (n, H, W, 3), from pinned_empty()); valid after the next sync().  rows: None or the ADDRESS of four int32 -- only these two
        runs of rows of every frame (the caller fills the others)."""
        if out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] or out.shape[1:] != (self.img_h, self.img_w, 3):
            raise ValueError("download_overlay_async needs a C-contiguous uint8 array (n, H, W, 3)")
        _check(self.lib.lt_download_overlay_rows_async(self._h, first, out.shape[0], out.ctypes.data, rows))

    def set_download_method(self, method):
        """-1: engine or kernel by measurement (default); 0: copy engine; 1: kernel."""
        _check(self.lib.lt_set_download_method(self._h, int(method)))

    def download_stats(self):
        eg, kg = C.c_double(), C.c_double()
        ec, kc, m = C.c_int(), C.c_int(), C.c_int()
        _check(self.lib.lt_download_stats(self._h, C.byref(eg), C.byref(ec), C.byref(kg), C.byref(kc), C.byref(m)))
        return {"engine_GBs": round(eg.value, 1), "engine_copies": ec.value, "kernel_GBs": round(kg.value, 1), "kernel_copies": kc.value,
                "method": "kernel" if m.value == 1 else "engine"}

    def store_overlay_device(self, sink, first=0, matrix="bt601"):
        """Enqueue the whole annotated frames of slots first .. first + len(sink) - 1 into `sink`, a device.DeviceFrames of this
        context's image size in any sink format -- RGB at its pitch, BGR / RGBA / BGRA (permuted, alpha 255), or NV12 / I420 converted
        with `matrix` ('bt601', 'bt709' or eight integers) -- behind the overlay_run / overlay_text that wrote them (lt_overlay_store_device).  Nothing crosses the
        bus.  The sink's memory is final after store_wait() or sync(); keep it alive until then."""
        if sink.img_size != (self.img_w, self.img_h):
            raise ValueError("expected a sink of %dx%d frames, got %dx%d" % ((self.img_w, self.img_h) + sink.img_size))
        layout = sink_format_id(sink.pixel_format)
        k = rgb2yuv_coeffs(matrix) if is_yuv(layout) else None
        s = np.ascontiguousarray(sink.surfaces)
        _check(self.lib.lt_overlay_store_device(self._h, int(first), s.shape[0], s.ctypes.data, layout, None if k is None else k.ctypes.data))
        return sink

    @staticmethod
    def _text_argument(n, lines_per_slot, origin, step, line_len):
        """-> (what keeps it alive, the address of the lt_inplace_text or None)."""
        text, keep = None, []
        if lines_per_slot is not None:
            if len(lines_per_slot) != n:
                raise ValueError("one list of text lines per slot")
            buf, nl = text_bytes(lines_per_slot, line_len)
            if nl:
                t = InplaceText(buf, nl, int(line_len), int(origin[0]), int(origin[1]), int(step))
                keep += [buf, t]
                text = C.addressof(t)
        return keep, text

    def overlay_run_to_surfaces_packed(self, ln, rn, lyx, ryx, sink, first=0, alpha=0.3, lines=None, origin=(20, 8), step=35, line_len=40,
                                       matrix="bt601"):
        """Lane and text drawn on the way from the camera frames of slots first .. first + len(sink) - 1 into `sink`, a
        device.DeviceFrames of this context's image size in 'rgb', 'nv12' or 'i420' (lt_overlay_run_to_surfaces): what overlay_run_packed
        + overlay_text + store_overlay_device leave there, in one pass and one launch per 32 slots whatever the slots' calibration sets.
        Only enqueued: the sink is final after store_wait() or sync(); keep it alive until then."""
        ln, rn = np.ascontiguousarray(ln, np.int32), np.ascontiguousarray(rn, np.int32)
        lyx, ryx = np.ascontiguousarray(lyx, np.int32), np.ascontiguousarray(ryx, np.int32)
        if len(rn) != len(ln) or lyx.size != 2 * int(ln.sum()) or ryx.size != 2 * int(rn.sum()):
            raise ValueError("point lists do not match their counts")
        if sink.img_size != (self.img_w, self.img_h):
            raise ValueError("expected a sink of %dx%d frames, got %dx%d" % ((self.img_w, self.img_h) + sink.img_size))
        if len(sink) != len(ln):
            raise ValueError("one surface per slot: %d surfaces for %d slots" % (len(sink), len(ln)))
        layout = draw_sink_format_id(sink.pixel_format)
        k = rgb2yuv_coeffs(matrix) if layout else None
        s = np.ascontiguousarray(sink.surfaces)
        keep, text = self._text_argument(len(ln), lines, origin, step, line_len)
        _check(self.lib.lt_overlay_run_to_surfaces(self._h, int(first), len(ln), ln.ctypes.data, rn.ctypes.data, lyx.ctypes.data if lyx.size else None,
                                                   ryx.ctypes.data if ryx.size else None, float(alpha), text, s.ctypes.data, layout,
                                                   None if k is None else k.ctypes.data))
        del keep
        return sink

    def overlay_run_to_surfaces(self, polygons, sink, first=0, **kw):
        """overlay_run_to_surfaces_packed for one (left_y, left_x, right_y, right_x) tuple per slot (empty arrays: no lane)."""
        return self.overlay_run_to_surfaces_packed(*pack_polygons(polygons), sink, first=first, **kw)

    def last_overlay_launches(self):
        """Lane-drawing kernel launches of the most recent overlay_run* / overlay_run_inplace* / overlay_run_to_surfaces*; -1: none yet."""
        return int(self.lib.lt_last_overlay_launches(self._h))

    def _inplace_tail(self, n, lines_per_slot, origin, step, line_len, matrix):
        """-> (what keeps the arguments alive, the address of the lt_inplace_text or None, the address of the eight integers or None)."""
        keep, text = self._text_argument(n, lines_per_slot, origin, step, line_len)
        k = None
        if self.input_format()[0] in PACKED_422:
            raise ValueError("packed 4:2:2 is an input format only: nothing is drawn into such surfaces")
        if self.input_format()[0] in RAW_FORMATS:
            raise ValueError("raw Bayer is an input format only: nothing is drawn into such surfaces")
        if self.input_format()[0] in RGB_FAMILY:
            raise ValueError("nothing is drawn into 'bgr' / 'rgba' / 'bgra' surfaces in place: such sinks are written by store_overlay_device")
        if pixel_format_id(self.input_format()[0]):
            if matrix is None:
                raise ValueError("drawing into 4:2:0 surfaces needs an RGB -> YUV matrix ('bt601', 'bt709' or eight integers)")
            k = rgb2yuv_coeffs(matrix)
            keep.append(k)
        return keep, text, None if k is None else k.ctypes.data

    def overlay_run_inplace_packed(self, ln, rn, lyx, ryx, first=0, alpha=0.3, lines=None, origin=(20, 8), step=35, line_len=40,
                                   matrix="bt601"):
        """Lane and text drawn INTO the surfaces attached to slots first .. (lt_overlay_run_inplace): the polygons packed as for
        overlay_run_packed, `lines` None or one list of strings per slot, `matrix` the RGB -> YUV matrix of a 4:2:0 context (not
        read by an RGB one).  Only enqueued: the surfaces are final after store_wait() or sync().  The slots are detached."""
        ln, rn = np.ascontiguousarray(ln, np.int32), np.ascontiguousarray(rn, np.int32)
        lyx, ryx = np.ascontiguousarray(lyx, np.int32), np.ascontiguousarray(ryx, np.int32)
        if len(rn) != len(ln) or lyx.size != 2 * int(ln.sum()) or ryx.size != 2 * int(rn.sum()):
            raise ValueError("point lists do not match their counts")
        keep, text, k = self._inplace_tail(len(ln), lines, origin, step, line_len, matrix)
        _check(self.lib.lt_overlay_run_inplace(self._h, int(first), len(ln), ln.ctypes.data, rn.ctypes.data, lyx.ctypes.data if lyx.size else None,
                                               ryx.ctypes.data if ryx.size else None, float(alpha), text, k))

    def overlay_run_inplace(self, polygons, first=0, **kw):
        """overlay_run_inplace_packed for one (left_y, left_x, right_y, right_x) tuple per slot (empty arrays: no lane)."""
        self.overlay_run_inplace_packed(*pack_polygons(polygons), first=first, **kw)

    def inplace_coeffs_available(self, n_rows):
        """Does overlay_run_inplace_coeffs exist for this context and this many plot rows (the limits of lt_overlay_run_strip_coeffs)?"""
        bh = self.warp_h
        return n_rows >= 1 and bh % 2 == 0 and bh * 4 >= 56 and (2 * bh + 2 * int(n_rows)) * 4 <= 60 * 1024

    def overlay_run_inplace_coeffs(self, coeffs, draw, ploty, ploty2, first=0, alpha=0.3, lines=None, origin=(20, 8), step=35, line_len=40,
                                   matrix="bt601"):
        """overlay_run_inplace_packed from the lanes' averaged coefficients (lt_overlay_run_inplace_coeffs): coeffs (n, 6) f64, draw
        (n,) u8 (0: no lane in that frame); plot points and polygon intervals are formed on the device."""
        coeffs = np.ascontiguousarray(coeffs, np.float64).reshape(-1, 6)
        draw = np.ascontiguousarray(draw, np.uint8)
        if len(draw) != len(coeffs):
            raise ValueError("one draw byte per frame")
        ploty, ploty2 = np.ascontiguousarray(ploty, np.float64), np.ascontiguousarray(ploty2, np.float64)
        keep, text, k = self._inplace_tail(len(coeffs), lines, origin, step, line_len, matrix)
        _check(self.lib.lt_overlay_run_inplace_coeffs(self._h, int(first), len(coeffs), coeffs.ctypes.data, draw.ctypes.data, ploty.ctypes.data,
                                                      ploty2.ctypes.data, len(ploty), float(alpha), text, k))

    def store_wait(self):
        """Block until every store_overlay_device and every overlay_run_inplace so far has landed -- and for nothing else."""
        _check(self.lib.lt_overlay_store_wait(self._h))

    def download_overlay_wait(self):
        """Block until the frames of every download_overlay_async have landed (later uploads / masks keep running)."""
        _check(self.lib.lt_download_overlay_wait(self._h))

    def download_bev(self, n, first=0):
        out = pinned_empty((n, self.warp_h, self.warp_w, 3))
        _check(self.lib.lt_download_bev(self._h, first, n, out.ctypes.data))
        return out

    # -- search visualisations, split-view panes (lt_search_viz_run & co.)
    def _viz_call(self, fn, items, fit_left, fit_right, band_left, band_right, out, shape):
        items = np.ascontiguousarray(items, VIZ_ITEM_DTYPE)
        n = int(items.shape[0])
        lists = [None if a is None else np.ascontiguousarray(a, np.int32).reshape(-1, 2) for a in (fit_left, fit_right, band_left, band_right)]
        fit, band = items["kind"] != 0, items["kind"] == 2          # (the library reads exactly these many points of each list)
        wants = (items["n_fit_left"][fit].sum(), items["n_fit_right"][fit].sum(), items["n_band_left"][band].sum(), items["n_band_right"][band].sum())
        for a, want in zip(lists, wants):
            if a is not None and a.shape[0] < int(want):
                raise ValueError("a point list is shorter than the items' counts")
        wait = out is None
        if wait:
            out = pinned_empty((n,) + shape)
        elif out.shape != (n,) + shape or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous uint8 array of shape %r" % ((n,) + shape,))
        _check(fn(self._h, n, items.ctypes.data, *[None if a is None else a.ctypes.data for a in lists], out.ctypes.data))
        if wait:
            self.search_viz_wait()
        return out

    def search_viz_run(self, items, fit_left=None, fit_right=None, band_left=None, band_right=None, out=None):
        """The search visualisations of the listed frames (`items`: VIZ_ITEM_DTYPE; the lists: int32 (y, x) pairs, the items' points
        back to back) -> (n, warp_h, warp_w, 3).  With `out` the call only enqueues: `out` is complete after search_viz_wait()."""
        return self._viz_call(self.lib.lt_search_viz_run, items, fit_left, fit_right, band_left, band_right, out, (self.warp_h, self.warp_w, 3))

    def split_panes_run(self, items, fit_left=None, fit_right=None, band_left=None, band_right=None, out=None):
        """The lower part of the split view of the listed frames -> (n, scaled_h, img_w, 3); otherwise as search_viz_run."""
        return self._viz_call(self.lib.lt_split_panes_run, items, fit_left, fit_right, band_left, band_right, out,
                              (self.split_panes_size()[1], self.img_w, 3))

    def split_panes_size(self):
        """(scaled_w, scaled_h, second_x) of triple_split_view for this context's camera and bird's-eye sizes."""
        a, b, c_ = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(self.lib.lt_split_panes_size(self._h, C.byref(a), C.byref(b), C.byref(c_)))
        return a.value, b.value, c_.value

    def search_viz_wait(self):
        """Block until the pictures of every search_viz_run / split_panes_run have landed (nothing else is waited for)."""
        _check(self.lib.lt_search_viz_wait(self._h))

    def resize_linear(self, img, dsize):
        """cv2.resize(img, dsize=(w, h)), INTER_LINEAR, on a u8 image of one or three channels (utils.resize_linear on the device)."""
        a = _u8(img)
        if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)):
            raise ValueError("resize_linear expects an (h, w) or (h, w, 3) image")
        ch = 1 if a.ndim == 2 else a.shape[2]
        dw, dh = int(dsize[0]), int(dsize[1])
        out = np.empty((dh, dw) if a.ndim == 2 else (dh, dw, ch), np.uint8)
        _check(self.lib.lt_resize_linear_u8(self._h, a.ctypes.data, a.shape[0], a.shape[1], ch, dh, dw, out.ctypes.data))
        return out

    def download_records(self, n, first=0):
        out = np.zeros(n, RECORD_DTYPE)
        _check(self.lib.lt_download_records(self._h, first, n, out.ctypes.data))
        return out

    def download_record(self, slot):
        """The record of one slot -> (left coeffs, right coeffs, detected, fit_flags): download_records(1, slot) without
        the per-call array and field lookups (LaneTracker.process() asks once per frame, with the device idle behind it)."""
        v = self.__dict__.get("_rec1")
        if v is None:
            r = np.zeros(1, RECORD_DTYPE)
            v = self._rec1 = (r, r.ctypes.data, r["left_coeffs"][0], r["right_coeffs"][0], r["detected"], r["fit_flags"])
        rc = self.lib.lt_download_records(self._h, slot, 1, v[1])
        if rc:
            _check(rc)
        return v[2].copy(), v[3].copy(), bool(v[4][0]), int(v[5][0])

    def overlay_rows(self):
        """(row0, row1): the camera rows in which the lane overlay can change a pixel (lt_overlay_rows)."""
        a, b = C.c_int(0), C.c_int(0)
        _check(self.lib.lt_overlay_rows(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def present_frame(self, slot, left_n, right_n, left_yx, right_yx, text, n_lines, line_len, out, rows=None, origin=(20, 8),
                      step=35, alpha=0.3):
        """draw_lane() / print_failure() of ONE slot in one library call (lt_present_frame), for a caller that keeps the packed
        polygon in buffers of its own: left_n / right_n / left_yx / right_yx are ADDRESSES (int32 count; int32 (y, x) pairs, or
        None when the count is 0), text is None or n_lines * line_len bytes (lines padded with NUL), out the (1, H, W, 3) array
        the frame lands in, rows None or the ADDRESS of four int32 {a0, a1, b0, b1}: only these two runs of rows are written."""
        rc = self.lib.lt_present_frame(self._h, slot, left_n, right_n, left_yx, right_yx, alpha, text, n_lines, line_len, origin[0],
                                       origin[1], step, out.ctypes.data, rows)
        if rc:
            _check(rc)
        return out

    def present_lane_async(self, slot, left_n, right_n, left_yx, right_yx, out, rows, alpha=0.3):
        """First half of present_frame (lt_present_lane_async): the polygon drawn, the rows the lane can reach on their way into
        `out`; no wait.  `rows` (address of four int32) is required."""
        rc = self.lib.lt_present_lane_async(self._h, slot, left_n, right_n, left_yx, right_yx, alpha, out.ctypes.data, rows)
        if rc:
            _check(rc)

    def present_lane_from_fit_async(self, slot, prev_sum_addr, count, ploty_addr, ploty2_addr, n_rows, out, rows, alpha=0.3):
        """The lane drawn by the device itself behind the slot's search (lt_present_lane_from_fit_async) -> True, or False where
        that form does not exist (LT_ERR_STATE: the caller draws once it has the record).  Addresses of f64 buffers the caller keeps."""
        rc = self.lib.lt_present_lane_from_fit_async(self._h, slot, prev_sum_addr, count, ploty_addr, ploty2_addr, n_rows, alpha,
                                                     out.ctypes.data, rows)
        if rc == -5:
            return False
        if rc:
            _check(rc)
        return True

    def lane_spans_from_fit(self, fit6, prev_sum, count, ploty, ploty2, detected=True, fit_flags=0):
        """Test hook (lt_lane_spans_from_fit): the row intervals (warp_h, 2) int16 the device forms for a fit given by value."""
        fit6 = np.ascontiguousarray(fit6, np.float64).reshape(6)
        ps = np.ascontiguousarray(prev_sum if prev_sum is not None else np.zeros(6), np.float64).reshape(6)
        ploty, ploty2 = np.ascontiguousarray(ploty, np.float64), np.ascontiguousarray(ploty2, np.float64)
        out = np.empty((self.warp_h, 2), np.int16)
        _check(self.lib.lt_lane_spans_from_fit(self._h, fit6.ctypes.data, int(bool(detected)), int(fit_flags), ps.ctypes.data, int(count),
                                               ploty.ctypes.data, ploty2.ctypes.data, len(ploty), out.ctypes.data))
        return out

    def present_finish(self, slot, text, n_lines, line_len, out, rows, origin=(20, 8), step=35):
        """Second half (lt_present_finish): the text lines, their rows into `out`, and the wait for both halves."""
        rc = self.lib.lt_present_finish(self._h, slot, text, n_lines, line_len, origin[0], origin[1], step, out.ctypes.data, rows)
        if rc:
            _check(rc)
        return out

    def download_pixels(self, slot, side):
        cnt = C.c_int(0)
        _check(self.lib.lt_download_pixels(self._h, slot, side, None, None, 0, C.byref(cnt)))
        n = cnt.value
        ys, xs = np.empty(n, np.int32), np.empty(n, np.int32)
        if n:
            _check(self.lib.lt_download_pixels(self._h, slot, side, ys.ctypes.data, xs.ctypes.data, n, C.byref(cnt)))
        return ys.astype(np.int64), xs.astype(np.int64)

    def download_centroids(self, slot, side):
        cap = self.info().max_levels + 2
        out = np.zeros(cap, np.int32)
        cnt = C.c_int(0)
        _check(self.lib.lt_download_centroids(self._h, slot, side, out.ctypes.data, cap, C.byref(cnt)))
        return [int(v) for v in out[:cnt.value]]

    def download_lane_lists(self, slot, want_centroids=True):
        """(left_y, left_x, right_y, right_x, left centroids or None, right centroids or None) of the slot's last search in ONE round
        trip to the device (lt_download_lane_lists); the lists are what download_pixels / download_centroids return."""
        cap = 1 << 16
        for _ in range(2):
            arrs = self.__dict__.get("_list_buf")
            if arrs is None or arrs[0].size < cap:
                arrs = self._list_buf = [np.empty(cap, np.int32) for _ in range(4)]       # (kept: 1 MB, filled by every call)
            cnt, ccnt = (C.c_int * 2)(), (C.c_int * 2)()
            ccap = self.info().max_levels + 2 if want_centroids else 0
            cl, cr = np.zeros(max(ccap, 1), np.int32), np.zeros(max(ccap, 1), np.int32)
            _check(self.lib.lt_download_lane_lists(self._h, int(slot), arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data,
                                                   arrs[0].size, cnt, int(bool(want_centroids)), cl.ctypes.data, cr.ctypes.data, ccap, ccnt))
            if max(cnt[0], cnt[1]) <= arrs[0].size:
                break
            cap = max(cnt[0], cnt[1])
        nl, nr = cnt[0], cnt[1]
        out = (arrs[0][:nl].astype(np.int64), arrs[1][:nl].astype(np.int64), arrs[2][:nr].astype(np.int64), arrs[3][:nr].astype(np.int64))
        if not want_centroids:
            return out + (None, None)
        return out + ([int(v) for v in cl[:ccnt[0]]], [int(v) for v in cr[:ccnt[1]]])

    def copy_records_to_device(self, n, dst_ptr, first=0):
        _check(self.lib.lt_copy_records_to_device(self._h, first, n, C.c_void_p(int(dst_ptr))))

    def enqueue_records_to_device(self, n, dst_ptr, first=0):
        """Stream-ordered copy (no host wait): valid in dst after the next sync()."""
        _check(self.lib.lt_enqueue_records_to_device(self._h, first, n, C.c_void_p(int(dst_ptr))))

    def set_frame_base(self, n, first_frame, first=0):
        _check(self.lib.lt_set_frame_base(self._h, first, n, int(first_frame)))

    # -- compute (asynchronous on the context's stream)
    def mask_run(self, n, fp=None, first=0, reuse_front=False):
        """undistort + warp + filter_lane_points over slots first .. first+n-1.  reuse_front: the slots' frames have been through
        mask_run already and only the filter parameters differ (the second try of a frame): lt_mask_rerun skips the front end where
        the slots' planes are still current."""
        fp = fp or filter_params()
        _check((self.lib.lt_mask_rerun if reuse_front else self.lib.lt_mask_run)(self._h, first, n, C.byref(fp)))

    def filter_run(self, n, fp=None, first=0):
        fp = fp or filter_params()
        _check(self.lib.lt_filter_run(self._h, first, n, C.byref(fp)))

    def sws_fit_run(self, n, sp=None, first=0):
        sp = sp or search_params()
        _check(self.lib.lt_sws_fit_run(self._h, first, n, C.byref(sp)))

    def band_fit_run(self, n, prev_coeffs, sp=None, first=0):
        sp = sp or search_params()
        prev = np.ascontiguousarray(prev_coeffs, np.float64).reshape(n, 6)
        _check(self.lib.lt_band_fit_run(self._h, first, n, C.byref(sp), prev.ctypes.data))

    def band_fit_chain_run(self, n, seed_coeffs=None, sp=None, first=0):
        """Band search + fit of slots first .. first+n-1 as consecutive frames of one stream, chained on the device:
        frame k+1 searches around frame k's fit; the first around `seed_coeffs` (6 doubles) or, if None, around the
        record of slot first-1.  Records behind a frame the chain could not build on come back with mode 255."""
        sp = sp or search_params()
        seed = None if seed_coeffs is None else np.ascontiguousarray(seed_coeffs, np.float64).reshape(6)
        _check(self.lib.lt_band_fit_chain_run(self._h, first, n, C.byref(sp), None if seed is None else seed.ctypes.data))

    def set_search_cus(self, n):
        """Reserve n CUs for the chained search (the compute streams are recreated without them); 0 undoes it."""
        _check(self.lib.lt_set_search_cus(self._h, int(n)))

    def set_walk_min_frames(self, frames):
        """Calls of at least `frames` frames take the walking threshold kernels (0: always; negative: the default, 80)."""
        _check(self.lib.lt_set_walk_min_frames(self._h, int(frames)))

    def set_direct_upload(self, on=-1):
        """One frame's rows (upload_frame_rows(enqueue=True) of a frame or two) stored by the calling thread through the PCIe
        aperture instead of copied by the engine: True / False allows / forbids, -1 asks.  -> does this context take the aperture?"""
        r = self.lib.lt_set_direct_upload(self._h, -1 if on == -1 else int(bool(on)))
        if r < 0:
            _check(r)
        return bool(r)

    def direct_upload_count(self):
        return int(self.lib.lt_direct_upload_count(self._h))

    def urgent(self):
        """Context manager: the stage calls inside run on the context's urgent stream (lt_set_urgent) -- behind the work of their
        own slots only, not behind masks of later frames already queued -- and downloads wait for that stream only."""
        import contextlib

        @contextlib.contextmanager
        def scope():                     # re-entrant: the mode ends with the outermost scope
            depth = getattr(self, "_urgent_depth", 0)
            if depth == 0:
                _check(self.lib.lt_set_urgent(self._h, 1))
            self._urgent_depth = depth + 1
            try:
                yield self
            finally:
                self._urgent_depth -= 1
                if self._urgent_depth == 0:
                    _check(self.lib.lt_set_urgent(self._h, 0))
        return scope()

    def band_fit_chain_cancel(self):
        """Chains enqueued so far stop at their next frame (their speculation has been rejected)."""
        _check(self.lib.lt_band_fit_chain_cancel(self._h))

    def band_fit_chain_collect(self, n, first=0):
        """Records of slots first .. first+n-1 as the most recent chain covering them left them; waits for that chain only."""
        out = np.zeros(n, RECORD_DTYPE)
        _check(self.lib.lt_band_fit_chain_collect(self._h, first, n, out.ctypes.data))
        return out

    # -- single-image operators
    def bilateral_adaptive_threshold(self, img, ksize, C_, mode, true_value, false_value):
        a = _u8(img)
        if a.ndim != 2:
            raise ValueError("bilateral_adaptive_threshold expects a single-channel image")
        out = np.empty_like(a)
        _check(self.lib.lt_bilateral_adaptive_threshold(self._h, a.ctypes.data, a.shape[0], a.shape[1], int(ksize),
                                                        int(C_), int(mode), int(true_value), int(false_value),
                                                        out.ctypes.data))
        return out

    def filter_lane_points(self, bev, fp=None):
        fp = fp or filter_params()
        a = _u8(bev)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("filter_lane_points expects an RGB image (H, W, 3)")
        out = np.empty(a.shape[:2], np.uint8)
        _check(self.lib.lt_filter_lane_points(self._h, a.ctypes.data, a.shape[0], a.shape[1], C.byref(fp),
                                              out.ctypes.data))
        return out

    def morph_ellipse(self, img, k, op, direct=False):
        """op: 'erode' | 'dilate' | 'tophat' | 'open' with the k x k ellipse (k in 5, 29, 55)."""
        a = _u8(img)
        if a.ndim != 2:
            raise ValueError("morph_ellipse expects a single-channel image")
        out = np.empty_like(a)
        code = {"erode": 0, "dilate": 1, "tophat": 2, "open": 3}[op]
        _check(self.lib.lt_morph_ellipse(self._h, a.ctypes.data, a.shape[0], a.shape[1], int(k), code,
                                         int(bool(direct)), out.ctypes.data))
        return out

    MORPH_FAMILIES = ("none", "one", "one_pair", "runs2", "split", "one_row")
    MORPH_OPS = {"erode": 0, "dilate": 1, "tophat": 2, "tophat_copy": 3}

    def morph_planes(self, planes, k, op, bands=0, padded=False, route=0):
        """Test hook (lt_morph_planes): one call of the top-hat launchers on `planes` (n, h, w) u8 -- route 1 (launch_morph_one_pair):
        (2, n, h, w), the 55x55 chain's planes and the 29x29 chain's.  op: 'erode' | 'dilate' | 'tophat' | 'tophat_copy'; bands 0 is the
        launcher's own rule; padded: a destination pitch of (w + 63) & ~63.  Returns a dict: `dst`, `mid` (the eroded intermediate of a
        top-hat, else None) and `copy` -- the WHOLE allocations, (n + 2, h, pitch) each ((2, n + 2, h, pitch) for route 1), 0xA5 wherever
        nothing was stored, the work in planes 1 .. n --, `launched`, and `report` (family, wide, nbands, band_rows, pair_strip, q,
        nbands29, band_rows29)."""
        a = _u8(planes)
        if a.ndim != (4 if route else 3) or (route and a.shape[0] != 2):
            raise ValueError("morph_planes expects (n, h, w) planes, or (2, n, h, w) for the pair route")
        n, h, w = a.shape[-3:]
        code = self.MORPH_OPS[op]
        pitch = (w + 63) & ~63 if padded else w
        lead = (2, n + 2) if route else (n + 2,)
        dst = np.empty(lead + (h, pitch), np.uint8)
        mid = np.empty(lead + (h, w), np.uint8)
        cp = np.empty(lead + (h, pitch), np.uint8)
        rep = (C.c_int32 * 8)()
        launched = C.c_int(0)
        _check(self.lib.lt_morph_planes(self._h, a.ctypes.data, n, h, w, int(k), code, int(bands), pitch if padded else 0, int(route),
                                        dst.ctypes.data, mid.ctypes.data, cp.ctypes.data, rep, C.byref(launched)))
        names = ("family", "wide", "nbands", "band_rows", "pair_strip", "q", "nbands29", "band_rows29")
        report = dict(zip(names, (int(v) for v in rep)))
        report["family"] = self.MORPH_FAMILIES[report["family"]]
        return dict(dst=dst, mid=mid if code >= 2 else None, copy=cp, launched=bool(launched.value), report=report)

    def fit_poly2(self, ys, xs):
        """np.polyfit(ys, xs, 2) on the device; rank-deficient inputs get NumPy's minimum-norm answer."""
        ys = np.ascontiguousarray(ys, np.int32)
        xs = np.ascontiguousarray(xs, np.int32)
        coef = (C.c_double * 3)()
        bad = C.c_int(0)
        _check(self.lib.lt_fit_poly2(self._h, ys.ctypes.data, xs.ctypes.data, int(ys.size), self.warp_h, self.warp_w,
                                     coef, C.byref(bad)))
        if bad.value:
            from .lane_tracker import _minimum_norm_parabola
            return _minimum_norm_parabola(ys, xs)
        return np.array(coef[:], np.float64)

    # -- measurement
    def timer_start(self):
        _check(self.lib.lt_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float(0)
        _check(self.lib.lt_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def set_stage_timing(self, enabled):
        _check(self.lib.lt_set_stage_timing(self._h, int(bool(enabled))))

    def last_threshold_path(self):
        """1 = long-walk threshold kernels, 0 = tile kernel, -1 = no bilateral chain has run yet."""
        return int(self.lib.lt_last_threshold_path(self._h))

    def last_threshold_form(self):
        """0 = tile kernel, 1 = running-sum walks, 2 = matrix-core form (i8 band products), -1 = no bilateral chain has run yet."""
        return int(self.lib.lt_last_threshold_form(self._h))

    def last_open_form(self):
        """5x5 open of the last slice launched: 0 = separate kernels, 1 = wave walk (k_merge_open5), 2 = small form (k_or_open5_small), -1 = none yet."""
        return int(self.lib.lt_last_open_form(self._h))

    def last_tophat_path(self):
        """Batch top-hat walks of the last mask chain: bit 0 = 29x29, bit 1 = 55x55 ran the split-band form; 0 = neither, -1 = none yet."""
        return int(self.lib.lt_last_tophat_path(self._h))

    def last_search_source(self):
        """What the last search call read: 1 = bit planes only, 0 = the u8 mask of at least one slot, -1 = no search yet."""
        return int(self.lib.lt_last_search_source(self._h))

    def last_adaptive_path(self):
        """'neighborhood' calls: 1 = running box sums, 0 = per-pixel windows, -1 = none yet."""
        return int(self.lib.lt_last_adaptive_path(self._h))

    def stage_reset(self):
        _check(self.lib.lt_stage_reset(self._h))

    def stage_ms(self):
        ms = (C.c_float * NUM_STAGES)()
        ln = (C.c_int32 * NUM_STAGES)()
        _check(self.lib.lt_stage_ms(self._h, ms, ln, NUM_STAGES))
        return {self.lib.lt_stage_name(i).decode(): (ms[i], ln[i]) for i in range(NUM_STAGES)}


class Gather:
    """The RCCL all-gather of lane records between the ranks of one node (lt_gather_*; one per rank, bound to
    the rank's Context).  Collective calls: every rank must make them in the same order."""

    def __init__(self, ctx, rank, world, id_path, timeout_s=120):
        self._g = None
        self.ctx, self.lib = ctx, ctx.lib
        g = _P()
        _check(self.lib.lt_gather_init(ctx._h, int(rank), int(world), os.fsencode(id_path), int(timeout_s), C.byref(g)))
        self._g = g
        self.rank, self.world = int(rank), int(world)

    def reserve(self, records_per_rank):
        _check(self.lib.lt_gather_reserve(self._g, int(records_per_rank)))

    def stage(self, n, at=0, first=0):
        """Records of slots [first, first+n) -> send buffer position `at`; stream-ordered, no host wait."""
        _check(self.lib.lt_gather_stage(self._g, int(first), int(n), int(at)))

    def records(self, n_records):
        """(world, n_records) records: the first n_records staged records of every rank."""
        out = np.zeros((self.world, int(n_records)), RECORD_DTYPE)
        _check(self.lib.lt_gather_records(self._g, int(n_records), out.ctypes.data))
        return out

    def host(self, array):
        """All-gather of a small host array: (world,) + array.shape."""
        a = np.ascontiguousarray(array)
        out = np.empty((self.world,) + a.shape, a.dtype)
        _check(self.lib.lt_gather_host(self._g, a.ctypes.data, a.nbytes, out.ctypes.data))
        return out

    def barrier(self):
        _check(self.lib.lt_gather_barrier(self._g))

    def close(self):
        if self._g is not None:
            self.lib.lt_gather_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count():
    n = C.c_int(0)
    _check(load().lt_device_count(C.byref(n)))
    return n.value


def lane_polygon_spans(warp_h, left_y, left_x, right_y, right_x):
    """(warp_h, 2) int16 (lo, hi) column interval per bird's-eye row of draw_lane's filled polygon
    (host-only helper of the overlay stage; rows the polygon does not touch are (32767, -32768))."""
    lyx = np.ascontiguousarray(np.stack([np.asarray(left_y), np.asarray(left_x)], 1).reshape(-1, 2), np.int32)
    ryx = np.ascontiguousarray(np.stack([np.asarray(right_y), np.asarray(right_x)], 1).reshape(-1, 2), np.int32)
    out = np.empty((int(warp_h), 2), np.int16)
    _check(load().lt_lane_polygon_spans(int(warp_h), lyx.ctypes.data if len(lyx) else None, len(lyx),
                                        ryx.ctypes.data if len(ryx) else None, len(ryx), out.ctypes.data))
    return out
