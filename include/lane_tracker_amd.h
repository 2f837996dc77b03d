/*
 * lane_tracker_amd.h -- C ABI of the MI355X-native lane-tracker hot path.
 *
 * The upstream reference (pierluigiferrari/lane_tracker) is pure Python and has no FFI of its own;
 * its boundary for this path is the Python API used by process_video.py.  This header is what a
 * maintainer binds with ctypes to replace the cv2/NumPy call sites on that path (INTEGRATION.md
 * shows the binding).  Each entry point cites the reference lines it replaces.
 *
 * Conventions: every function returns 0 on success and a negative lt_status on failure;
 * lt_last_error() returns a thread-local description.  No exceptions cross the ABI, no torch or
 * HIP types appear in signatures.  A context owns one HIP stream and all of its device buffers;
 * contexts are not thread-safe (one per tracker / per rank).  Host buffers are caller-owned.
 * The library is HIP-only: there is no CPU fallback behind any entry point.
 *
 * Frame "slots": a context holds `capacity` (lt_reserve) independent frame slots in HBM.  Slot i
 * keeps the camera frame, every intermediate plane, the mask, the lane-pixel lists and the 64-byte
 * lane record of frame i.  The *_run functions enqueue kernels on the context's stream and return
 * immediately; downloads synchronise.
 */
#ifndef LANE_TRACKER_AMD_H
#define LANE_TRACKER_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden; the declarations below are its whole export list
 * (tests/test_native_abi.py compares `nm -D` with this header). */
#pragma GCC visibility push(default)

/* 2: + lt_gather_*, lt_band_fit_chain_run, lt_calib_*, lt_upload_frame_rows_async & co.; lt_debug_cycles removed;
 *    lt_last_threshold_path(NULL) returns LT_NO_CONTEXT instead of -1. */
/* 3: + lt_present_frame, lt_present_lane_async, lt_present_finish, lt_overlay_rows, lt_upload_frame_rest_rows (one frame per
 *    call, the host waiting: LaneTracker.process()), lt_set_download_method, lt_download_stats, lt_device_cache_trim,
 *    lt_last_adaptive_path, lt_host_copy_async, lt_host_copy2d_async, lt_host_copy_wait, lt_overlay_run_rows,
 *    lt_download_overlay_rows_async.  Nothing removed or changed. */
/* 4: + lt_host_copy_group_create / _destroy, lt_host_copy_async_group, lt_host_copy2d_async_group, lt_host_copy_wait_group
 *    (completion per group instead of per process), lt_shutdown, lt_device_cache_stats, lt_warm (a stream's set-up ahead of its
 *    first window), lt_overlay_run_strip + lt_strip_download_async (annotated frames as one packed strip of rows per frame through
 *    page-locked staging blocks into ordinary memory), lt_text_blend_host + lt_host_text_async_group (the text lines on the host),
 *    lt_host_copy_stats, lt_host_touch_async_group; lt_upload_frame_rows_enqueue (an upload nobody waits for),
 *    lt_present_lane_from_fit_async + lt_lane_spans_from_fit (the lane of a frame drawn by the device behind its search),
 *    lt_overlay_run_strip_coeffs (strips from averaged coefficients).  Nothing removed or changed. */
/* 5: + lt_device_cache_counters (hits / misses / evictions of the device-memory cache since the process started),
 *    lt_set_walk_min_frames (the batch size from which the threshold stage takes its walking kernels; was an environment
 *    switch), lt_host_memory_stats, lt_mask_rerun (a second parameter set over frames whose front end has run), lt_download_lane_lists (a search's lists in one
 *    round trip), lt_set_direct_upload + lt_direct_upload_count (one frame's rows stored through the PCIe aperture),
 *    lt_host_text_now_group (a frame's text lines drawn at once, behind the group's copies), lt_frame_tail (validity, average,
 *    plot points, radius and eccentricity of a valid first try in one host call).  Later additions, still 5:
 *    lt_search_item + lt_search_fit_list (the searches of frames of unrelated streams in one launch), lt_upload_frame_rows_list +
 *    lt_upload_frame_rest_list (the uploads of frames that lie in separate host arrays); lt_set_input_format + lt_get_input_format +
 *    lt_yuv_to_rgb (camera frames in YUV 4:2:0, NV12 or I420, or packed 4:2:2, YUY2 or UYVY, converted on the device), lt_bayer_to_rgb (8-bit raw Bayer, layouts 16 .. 19, demosaiced on the device); lt_device_surface + lt_attach_device_frames +
 *    lt_device_frames_rest (camera frames that already lie in device memory, read where they lie), lt_device_alloc / _free /
 *    _write / _read (device blocks for callers without a HIP binding of their own), lt_device_stream_wait; lt_viz_item +
 *    lt_search_viz_run + lt_split_panes_run + lt_split_panes_size + lt_search_viz_wait (the search visualisations and split-view
 *    panes of listed frames, painted on the device), lt_calib_split_panes_size, lt_resize_linear_u8; lt_rgb_to_surfaces + lt_overlay_store_device +
 *    lt_overlay_store_wait (annotated frames written into the caller's device surfaces, RGB, NV12 or I420); lt_add_calibration +
 *    lt_calibration_count + lt_set_slot_calibrations + lt_get_slot_calibrations + lt_overlay_configure_set (several calibrations in
 *    one context, one per slot: the cameras of a LaneTrackerGroup); lt_inplace_text + lt_overlay_run_inplace +
 *    lt_overlay_run_inplace_coeffs (lane and text drawn into the attached camera surfaces themselves); lt_overlay_run_to_surfaces +
 *    lt_last_overlay_launches (lane and text drawn on the way into device sinks, one launch whatever the slots' calibration sets);
 *    lt_set_input_size + lt_get_input_size + lt_get_input_rows (RGB camera frames of another size than the calibration's, resized on
 *    the device); lt_set_raw_lut + lt_get_raw_lut (black level, white balance and tone curve of raw Bayer input as one table per colour
 *    phase, looked up on the device inside the undistortion and the row conversion); lt_set_raw_lut_wide + lt_get_raw_lut_wide +
 *    lt_raw16_to_rgb (10- and 12-bit raw Bayer, layouts 32 .. 35 and 48 .. 51: 16-bit words looked up in a table of 1 << bits entries per
 *    colour phase on their way into the 8-bit demosaic); lt_set_raw_color + lt_get_raw_color + lt_raw_to_rgb_color (the colour stage of raw
 *    Bayer input: a colour-correction matrix and an output curve on every demosaiced pixel, on the device); lt_set_raw_shading +
 *    lt_get_raw_shading + lt_get_raw_shading_plane + lt_raw_to_rgb_shaded (lens-shading correction of raw Bayer input from a gain mesh, on
 *    every sample in front of the raw table, on the device); lt_upload_mask_bits + lt_last_search_source (caller-supplied masks as
 *    bit planes, searched by the bit-plane kernels); lt_last_open_form (which form of the 5x5 open a mask run's last slice took);
 *    lt_add_raw_set + lt_raw_set_count + lt_set_slot_raw_sets + lt_get_slot_raw_sets + lt_set_raw_lut_of + lt_get_raw_lut_of +
 *    lt_set_raw_color_of + lt_get_raw_color_of + lt_set_raw_shading_of + lt_get_raw_shading_of + lt_get_raw_shading_plane_of +
 *    lt_last_raw_walk_form (raw table, colour stage and shading map per slot: several raw sets in one context).
 *    Nothing removed or changed. */
#define LT_ABI_VERSION 5

typedef enum lt_status {
    LT_OK = 0,
    LT_ERR_INVALID = -1,     /* bad argument (also the reference's ValueError cases) */
    LT_ERR_HIP = -2,         /* a HIP runtime call failed */
    LT_ERR_NOMEM = -3,
    LT_ERR_CAPACITY = -4,    /* slot range outside lt_reserve()'d capacity */
    LT_ERR_STATE = -5        /* e.g. search requested before a mask exists */
} lt_status;

typedef struct lt_ctx lt_ctx;

/* LaneTracker.__init__ arguments that shape the kernels (lane_tracker.py:101-137). */
typedef struct lt_calib {
    int32_t img_w, img_h;        /* img_size     (width, height) */
    int32_t warp_w, warp_h;      /* warped_size  (width, height) */
    double  cam_matrix[9];       /* row major */
    double  dist_coeffs[5];      /* k1 k2 p1 p2 k3 */
    double  M[9];                /* warp_matrices[0]: camera -> bird's eye */
} lt_calib;

/* filter_lane_points() keyword arguments (lane_tracker.py:183-193). */
typedef struct lt_filter_params {
    int32_t filter_type;         /* 0 'bilateral', 1 'neighborhood'; anything else -> LT_ERR_INVALID (:220) */
    int32_t ksize_r, C_r, ksize_b, C_b;
    int32_t mask_noise, noise_thresh, ksize_noise, C_noise;
} lt_filter_params;

/* sliding_window_search() / band_search() arguments (lane_tracker.py:242-253, 449). */
typedef struct lt_search_params {
    int32_t window_width, window_height, search_range, no_success_limit;
    int32_t ignore_sides, ignore_bottom, bandwidth, _pad;
    double  mu, start_slice, partial;
} lt_search_params;

/* One fitted frame, 64 bytes; this is the unit the multi-GPU gather moves. */
typedef struct lt_lane_record {
    double  left_coeffs[3];      /* np.polyfit order: x = a*y^2 + b*y + c (lane_tracker.py:506) */
    double  right_coeffs[3];     /* (:507) */
    int32_t n_left, n_right;     /* lane-pixel counts */
    uint8_t detected;            /* self.detected_pixels (:438, :496) */
    uint8_t fit_flags;           /* bit0: left fit rank-deficient (<3 distinct y), bit1: right */
    uint8_t mode;                /* 0 sliding-window, 1 band, 255 not searched (lt_band_fit_chain_run stopped before it) */
    uint8_t _pad;                /* reserved (the library records how the slot's lane pixels are stored) */
    int32_t frame;               /* caller-defined global frame index */
} lt_lane_record;

/* One frame of a search list (lt_search_fit_list), 64 bytes: the slot its mask is in, the search it gets (0 sliding window,
 * 1 band) and, for a band search, the coefficients its band is drawn around (last_left_coeffs, last_right_coeffs). */
typedef struct lt_search_item {
    int32_t slot;
    int32_t mode;
    int32_t _pad[2];
    double  prev_coeffs[6];
} lt_search_item;

/* One frame of a visualisation list (lt_search_viz_run, lt_split_panes_run), 48 bytes: the slot whose mask, lane pixels and window
 * centroids are shown, which picture (lane_tracker.py:1130-1137) and the parameters of the search that is shown. */
typedef struct lt_viz_item {
    int32_t slot;
    int32_t kind;                      /* 0 the bare mask (nothing detected), 1 sliding-window search, 2 band search */
    int32_t window_width, window_height, ignore_bottom;   /* kind 1 */
    int32_t bandwidth;                                    /* kind 2 */
    int32_t n_fit_left, n_fit_right;   /* plot points of the new fit (kinds 1, 2) */
    int32_t n_band_left, n_band_right; /* kind 2: plot points of the curves the band was searched around */
    int32_t _pad[2];
} lt_viz_item;

typedef struct lt_info {
    int32_t abi_version, device, capacity, cu_count;
    int32_t src_row0, src_row1;  /* camera rows [row0,row1) that influence the bird's-eye view */
    int32_t max_pixels_per_side; /* capacity of each lane-pixel list */
    int32_t max_levels;          /* capacity of each centroid list */
    int64_t alg_bytes_mask;      /* algorithmic bytes / frame of the warp+threshold stage */
    int64_t alg_bytes_search;    /* algorithmic bytes / frame of search+fit, excluding emitted pixels */
    char    device_name[64];
} lt_info;

enum lt_plane {                  /* lt_download_plane selectors (bird's-eye planes, h*w bytes each) */
    LT_PLANE_R = 0,              /* rgb_r_channel        (:207) */
    LT_PLANE_LAB_B = 1,          /* lab_b_channel        (:208) */
    LT_PLANE_TOPHAT_R = 2,       /* rgb_r_tophat         (:210) */
    LT_PLANE_TOPHAT_B = 3,       /* lab_b_tophat         (:211) */
    LT_PLANE_MERGED = 4,         /* merged               (:229-235) */
    LT_PLANE_MASK = 5            /* opened = return value (:238) */
};

#define LT_NUM_STAGES 12         /* lt_stage_ms slots, see lt_stage_name() */

/* ---- lifecycle ------------------------------------------------------------------------------- */
const char* lt_last_error(void);
int  lt_abi_version(void);
int  lt_device_count(int* count);
/* Builds the calibration-constant tables (remap tables, Lab LUTs, structuring elements) on the
 * host in f64 and uploads them.  Replaces the per-call table work inside cv2.undistort /
 * cv2.warpPerspective / cv2.cvtColor / cv2.getStructuringElement (:203-205, :208, :832, :834). */
int  lt_create(const lt_calib* calib, int device, lt_ctx** out);
void lt_destroy(lt_ctx* ctx);
int  lt_reserve(lt_ctx* ctx, int capacity);
/* Set-up ahead of use, for the current capacity (call lt_reserve first): the streams, page-locked staging and device buffers that
 * the first searches / the first chained search / the first overlay would otherwise create on the way (20-35 ms of the first
 * window of a stream).  sws / band: the search parameters to size the result buffers for (either may be NULL); annotate: 0 = no
 * presentation stage, 1 = whole annotated frames (lt_overlay_run), 2 = strips (lt_overlay_run_strip); needs lt_overlay_configure
 * for 1 and 2; + 4: the staging ring of lt_search_viz_run, + 8: that of lt_split_panes_run as well.  Optional: every entry point
 * still sets up what it finds missing.  LT_ERR_INVALID for search parameters the search calls themselves refuse (the size limits
 * at lt_sws_fit_run). */
int  lt_warm(lt_ctx* ctx, const lt_search_params* sws, const lt_search_params* band, int annotate);
int  lt_get_info(lt_ctx* ctx, lt_info* out);
int  lt_sync(lt_ctx* ctx);
/* Number of HIP streams (1..8, default 1) the context spreads its slots over.  Slot s always runs on
 * stream s*k/capacity, so the stages of one frame stay ordered while slices overlap: the latency-bound
 * search of one slice hides under the mask chain of another.  Every transfer / sync waits for all streams. */
int  lt_set_streams(lt_ctx* ctx, int nstreams);

/* ---- frames in, results out ------------------------------------------------------------------ */
/* The pixel format of the camera frames a context takes: RGB interleaved (the default), or YUV 4:2:0 as cameras and decoders hand
 * it out -- NV12 (img_h rows of Y, then img_h / 2 rows of interleaved U,V pairs) or I420 (Y plane, U plane, V plane): one block
 * of img_h * 3 / 2 rows of img_w bytes, img_h * img_w * 3 / 2 bytes a frame.  Such frames are converted on the device, with
 * OpenCV's integer arithmetic (cv2.cvtColor(frame, COLOR_YUV2RGB_NV12 / _I420): one (U, V) pair per 2 x 2 block, 20-bit fixed point)
 *     y = max(0, Y - 16) * CY;   r = clamp((y + 2^19 + CVR (V - 128)) >> 20),   g = clamp((y + 2^19 + CVG (V - 128) + CUG (U - 128)) >> 20),
 *     b = clamp((y + 2^19 + CUB (U - 128)) >> 20)
 * and coeffs = {CY, CVR, CVG, CUG, CUB} (LT_YUV_BT601: OpenCV's own; LT_YUV_BT709; any other matrix whose magnitudes stay below
 * 2^23 and whose sums stay inside 32 bits).  lt_set_input_format is called once, before the context's first upload: LT_ERR_INVALID
 * for an unknown layout, missing or oversized coefficients or an odd img_w / img_h, LT_ERR_STATE for a change after an upload
 * (a context is one camera).  coeffs is not read for LT_INPUT_RGB.  In a 4:2:0 context every upload entry point below keeps its
 * name and meaning and takes 4:2:0 frames where it says frames_rgb: the lt_upload_frame_rows family moves the rows
 * [row0, row1) of the Y plane and the chroma rows under them (half the bytes of the RGB form), the undistortion converts the
 * taps it reads, and lt_upload_frames / the lt_upload_frame_rest family also leave the RGB form of the rows they bring in the
 * slot's camera frame, so that overlays, presentation and downloads find what they find in an RGB context.  Everything behind
 * the undistortion is bit for bit what an RGB context computes from the converted frames.
 * lt_get_input_format reads the setting back (coeffs may be NULL).
 * lt_yuv_to_rgb converts one host frame of h x w (even, at most 16384 each) on the device: out_rgb = h * w * 3 bytes.
 *
 * Packed YUV 4:2:2 as cameras and capture cards hand it out -- LT_INPUT_YUY2 (bytes Y0 U Y1 V; UVC webcams, SDI / HDMI capture) and
 * LT_INPUT_UYVY (U Y0 V Y1; GMSL / FPD-Link cameras): one plane of img_h rows of 2 * img_w bytes, img_h * img_w * 2 bytes a frame,
 * OpenCV's CV_8UC2.  The same arithmetic and coefficients with one (U, V) pair per horizontal pixel pair
 * (cv2.cvtColor(frame, COLOR_YUV2RGB_YUY2 / _UYVY)); img_w even and at least 4, img_h any.  Everything said above for 4:2:0 holds
 * with "rows [row0, row1) of the one plane" for the rows that are moved (2 / 3 of the bytes of the RGB form); lt_yuv_to_rgb takes a
 * frame of h * w * 2 bytes (w even, at least 4; any h).  4:2:2 is an INPUT format only: lt_rgb_to_surfaces and
 * lt_overlay_store_device return LT_ERR_INVALID for these two layouts, and lt_overlay_run_inplace* on a 4:2:2 context returns
 * LT_ERR_STATE before anything is staged (a 4:2:2 context writes its annotated frames into RGB, NV12 or I420 sinks like any other).
 *
 * The other members of the RGB family, as users' own software holds frames -- LT_INPUT_BGR (bytes B G R; OpenCV's cv2.imread /
 * VideoCapture: img_h rows of 3 * img_w bytes, numpy (H, W, 3)), LT_INPUT_RGBA (R G B A) and LT_INPUT_BGRA (B G R A; GStreamer / V4L2
 * RGBx / BGRx, capture and compositor surfaces: img_h rows of 4 * img_w bytes, numpy (H, W, 4)).  A channel permutation, folded
 * into the constant shifts the undistortion takes its channels out with: no conversion, `coeffs` is not read (NULL), the alpha
 * byte is never read, and everything is bit for bit what an RGB context computes from the permuted frames.  img_w at least 2, no
 * parity requirement.  Uploads and attached surfaces work as said above with one plane of 3 / 4 bytes a pixel (pitch >= 3 / 4 *
 * img_w; chroma_pitch is not read); lt_set_direct_upload returns 0 (rows go to staging).  These three are SINKS too:
 * lt_rgb_to_surfaces and lt_overlay_store_device write them (alpha = 255, bytes between a row's end and the pitch untouched, any
 * byte alignment).  Not supported: lt_overlay_run_inplace* on such a context and lt_set_input_size with such a format return
 * LT_ERR_STATE, lt_overlay_run_to_surfaces with such a sink layout LT_ERR_INVALID; lt_yuv_to_rgb does not take them.
 *
 * 8-bit raw Bayer, as a sensor delivers it before any image signal processor has run (machine-vision and GMSL cameras in raw mode,
 * raw sensor logs) -- LT_INPUT_BAYER_RGGB, _GRBG, _GBRG, _BGGR, named by the sensor's top-left 2 x 2 block: one plane of img_h rows
 * of img_w bytes, img_h * img_w bytes a frame (a third of the RGB form), numpy (H, W); img_w and img_h even and at least 4.  The
 * pixel at (y, x) carries the colour at position 2 * (y & 1) + (x & 1) of the pattern's name.  Demosaiced on the device, bilinear, in
 * integers -- at an interior pixel (1 <= y <= img_h - 2, 1 <= x <= img_w - 2) of the mosaic m:
 *     red / blue site:  own colour m[y,x];  G = (m[y-1,x] + m[y+1,x] + m[y,x-1] + m[y,x+1] + 2) >> 2;
 *                       the opposite colour = (m[y-1,x-1] + m[y-1,x+1] + m[y+1,x-1] + m[y+1,x+1] + 2) >> 2
 *     green site:       G = m[y,x];  the horizontal neighbours' colour = (m[y,x-1] + m[y,x+1] + 1) >> 1;
 *                       the vertical neighbours' colour = (m[y-1,x] + m[y+1,x] + 1) >> 1
 * and a border pixel takes the value of the interior pixel at (clamp(y, 1, img_h - 2), clamp(x, 1, img_w - 2)).  This is what
 * cv2.cvtColor(frame, COLOR_BayerRGGB2RGB / GRBG / GBRG / BGGR) is understood to compute; that was not checked against OpenCV, the
 * definition here is the contract.  `coeffs` is not read (NULL).  The undistortion demosaics the taps it reads, and everything
 * behind it is bit for bit what an RGB context computes from the demosaiced frames.  Uploads and attached surfaces work as said
 * above with one plane of one byte a pixel (pitch >= img_w; chroma_pitch is not read); the lt_upload_frame_rows family moves the
 * source rows that the windows of the path's camera rows touch (lt_get_input_rows: the run widened by a row on either side, four
 * rows at the least); lt_set_direct_upload returns 0.  lt_bayer_to_rgb is the conversion alone, of one host frame of h x w (even,
 * 4 .. 16384 each) on the device: out_rgb = h * w * 3 bytes.  Raw Bayer is an INPUT format only: lt_rgb_to_surfaces,
 * lt_overlay_store_device and lt_overlay_run_to_surfaces return LT_ERR_INVALID for these layouts, lt_overlay_run_inplace* on such a
 * context and lt_set_input_size with such a format return LT_ERR_STATE; lt_yuv_to_rgb does not take them.
 * A RAW TABLE conditions the samples before the demosaic: black-level subtraction, per-colour gains (white balance) and a tone curve are
 * together one 256-entry table per colour of the mosaic.  `lut` is uint8[4][256] (1024 bytes), indexed by the colour phase of a site --
 * 0: a red site, 1: green on a red row, 2: green on a blue row, 3: a blue site (phase = 2 * ((y ^ red_row) & 1) + ((x ^ red_col) & 1), the
 * red sites of RGGB / GRBG / GBRG / BGGR at (row, column) parity (0,0) / (0,1) / (1,0) / (1,1)) -- and the conditioned mosaic is
 *     s'(y, x) = lut[phase(y, x)][s(y, x)];
 * everything above is computed on s', the demosaic and its border rule included.  Whatever a context with table L computes from frames F
 * -- undistorted rows, planes, masks, records, camera frames, annotated frames, visualisations -- is bit for bit what the same context
 * without a table computes from the frames conditioned on the host.  lt_set_raw_lut(ctx, lut) sets the table, NULL removes it; it is allowed
 * before and after uploads, waits for everything the context has in flight (as lt_sync does), then writes the device copy, and governs every
 * undistortion and row conversion launched afterwards (what was computed before stays as it is; a front end is not reused across the
 * call).  It is a set-up call, or an occasional one -- an auto-white-balance step between windows -- NOT a per-frame call: it stalls the
 * context.  With a table set the conditioned kernels run whatever the table holds, the identity included; with none, the plain ones.
 * LT_ERR_STATE in a context whose input format is not raw Bayer; lt_set_input_format with a layout that is not raw Bayer removes the table.
 * lt_get_raw_lut: *is_set := 0 / 1 and, where one is set, the table into `lut` (either may be NULL).  Slots, uploads and lt_bayer_to_rgb are
 * unaffected.  Not built: 14 / 16-bit or companded raw (10 and 12 bits: below), other demosaics, a table
 * per slot (the colour-correction matrix: THE COLOUR STAGE, below).
 *
 * 10- AND 12-BIT RAW BAYER, as most raw sensors deliver it (GMSL / FPD-Link cameras in raw mode, BayerRG10 / BayerRG12, V4L2 SRGGB10 /
 * SRGGB12) -- LT_INPUT_BAYER10_RGGB .. _BGGR (32 .. 35) and LT_INPUT_BAYER12_RGGB .. _BGGR (48 .. 51), the pattern is layout & 3 in the
 * order above: one plane of img_h rows of img_w little-endian 16-bit words, 2 * img_h * img_w bytes a frame, numpy uint16 (H, W); img_w and
 * img_h even and at least 4.  A sample is the LOW `bits` (10 / 12) bits of its word; THE BITS ABOVE ARE IGNORED (masked off, never
 * checked).  Such a context ALWAYS has a table, `lut` = uint8[4][1 << bits], phase-major as above, and
 *     s'(y, x) = lut[phase(y, x)][F(y, x) & ((1 << bits) - 1)]
 * is an 8-bit mosaic: everything such a context computes from frames F is bit for bit what an 8-bit raw Bayer context of the same pattern
 * without a table computes from s'.  The mask is what keeps every index inside the table, which the kernels hold in LDS (4 KB / 16 KB a
 * workgroup).  lt_set_input_format(ctx, 32 .. 35 | 48 .. 51, NULL) applies the size rules of 8-bit raw Bayer, sizes the staging frames and
 * installs the DEFAULT table, lut[p][s] = floor(255 * s / ((1 << bits) - 1) + 0.5) (full scale to full scale, rounded; no black level, no
 * gains, no curve).  lt_set_raw_lut_wide(ctx, lut, entries) sets another one -- `entries` must be 1 << bits of the context's layout
 * (LT_ERR_INVALID), lut = NULL restores the default --, lt_get_raw_lut_wide reads the table in effect back; both return LT_ERR_STATE in a
 * context whose layout is not one of these, as lt_set_raw_lut does in a context whose layout is.  Like lt_set_raw_lut the setter waits for
 * everything the context has in flight and is a set-up or occasional call, NOT a per-frame one.  Uploads (all of them) and attached surfaces
 * work as for 8-bit raw Bayer with two bytes a pixel: pitch >= 2 * img_w, and the plane's address and the pitch must be EVEN
 * (LT_ERR_INVALID).  lt_raw16_to_rgb is the conversion alone, lt_bayer_to_rgb's twin: one host frame of h x w words, `lut` = 4 << bits bytes
 * or NULL for the default.  Input formats only, as 8-bit raw Bayer is, with the same refusals.  Not built: 14 and
 * 16 bits, MSB-aligned containers, a table per stream.
 *
 * MIPI-PACKED RAW10 / RAW12, as a CSI-2 receiver writes it (a deserialiser's DMA engine, a raw sensor log; V4L2 SRGGB10P / SRGGB12P and their
 * siblings) -- LT_INPUT_BAYER10P_RGGB .. _BGGR (36 .. 39) and LT_INPUT_BAYER12P_RGGB .. _BGGR (52 .. 55): the pattern stays layout & 3, bit 2
 * says packed.  One plane of bytes, numpy uint8 (H, row bytes):
 *   RAW10  img_w % 4 == 0; a row is 5 * img_w / 4 bytes.  Group g holds sites 4g .. 4g + 3: byte 5g + i is s[4g + i] >> 2 for i = 0 .. 3, and
 *          bits 2i + 1 : 2i of byte 5g + 4 are s[4g + i] & 3.
 *   RAW12  img_w even; a row is 3 * img_w / 2 bytes.  Byte 3g is s[2g] >> 4, byte 3g + 1 is s[2g + 1] >> 4, and byte 3g + 2 is
 *          (s[2g] & 15) | (s[2g + 1] & 15) << 4.
 * img_h is even and at least 4, as for every raw layout (img_w at least 4 too).  A surface's pitch may be any value that is at least the row
 * bytes, at ANY byte alignment of plane and pitch.  No bits lie above the sample, so nothing is masked or ignored.  The samples are unpacked
 * in the kernels, on their way into the lookups: no pass over the frame, no repack on the device, 1.25 / 1.5 bytes a sample over the bus.
 * Everything a context in one of these layouts with table L (and, optionally, a colour stage and a shading map) computes from packed frames
 * F -- undistorted rows, planes, masks, records, camera frames, annotated frames, states -- is BIT FOR BIT what the context of the 16-bit
 * layout (layout & ~4) with the same table, stage and map computes from the unpacked frames (utils.unpack_raw, which is the definition).
 * lt_set_input_format refuses img_w % 4 != 0 (RAW10), an odd img_w or img_h and sizes below 4 (LT_ERR_INVALID), and on a context with an input
 * size these layouts are LT_ERR_INVALID too (the 16-bit layouts: LT_ERR_STATE) -- layouts 36 .. 39 and 52 .. 55 were no layouts there before,
 * and what they answered is kept; lt_set_raw_lut_wide,
 * lt_set_raw_color and lt_set_raw_shading work as for the 16-bit layouts; lt_raw_to_rgb_color / lt_raw_to_rgb_shaded take these layouts with
 * `frame` = h dense packed rows (lt_raw16_to_rgb does not: its frame is words).  Input formats only, with the refusals of the other raw
 * layouts.  Not built: 14- and 16-bit samples, RAW14 packing, MSB-aligned words, big-endian or line-padded CSI-2 framing beyond a plain
 * pitch, packed sinks, a table, stage or map per stream of a group.
 *
 * THE COLOUR STAGE of raw Bayer input, 8-, 10- and 12-bit alike: what an image signal processor does AFTER the demosaic, where the raw
 * table cannot reach because it mixes channels -- a colour-correction matrix from sensor RGB to display RGB, then one output curve.  `ccm`
 * is int16[9], row-major, in Q10 (1024 is 1.0; row c makes output channel c), `curve` uint8[256]; for a demosaiced pixel (R, G, B)
 *     v[c]   = (ccm[3c] * R + ccm[3c + 1] * G + ccm[3c + 2] * B + 512) >> 10        (int32, arithmetic shift: floor)
 *     out[c] = curve[min(max(v[c], 0), 255)]
 * Any int16 matrix is legal (3 * 255 * 32768 < 2^31).  Everything a context with stage (ccm, curve) computes from frames F -- undistorted
 * rows, planes, masks, records, camera frames, annotated frames, visualisations -- is bit for bit what an RGB context computes from the
 * demosaiced (and, with a raw table, conditioned) frames taken through the two lines above on the host.  In the undistortion the stage is
 * applied to each demosaiced tap BEFORE the bilinear blend (clamp and curve are not linear); taps outside the image are 0 after it, as ever.
 * So the camera's order is expressible: black level and white balance in the raw table (linear, no tone curve there), demosaic, matrix on
 * linear data, gamma in `curve`.  lt_set_raw_color(ctx, ccm, curve, enable): enable != 0 sets the stage, ccm = NULL the identity matrix
 * (1024 on the diagonal), curve = NULL the identity curve; enable = 0 removes it (neither pointer is read) and the plain raw kernels run
 * again.  With a stage set its kernels run whatever it holds, the identity included.  Like lt_set_raw_lut it waits for everything the context
 * has in flight, governs what is launched afterwards, and is a set-up or occasional call, NOT a per-frame one; the raw table may be set or
 * changed before or after it.  LT_ERR_STATE in a context whose input format is not raw Bayer; lt_set_input_format with another layout
 * removes the stage.  lt_get_raw_color: *is_set := 0 / 1 and, where one is set, matrix and curve into `ccm` / `curve` (any may be NULL).
 * lt_raw_to_rgb_color is the conversion alone with the stage, of one host frame of h x w in any of the twelve raw layouts (bytes, or 16-bit
 * words for 10 / 12 bits): `lut` the raw table of 4 * lut_entries bytes (256, or 1 << bits; LT_ERR_INVALID otherwise) or NULL -- none
 * for 8-bit, the default for 10 / 12 --, ccm / curve as above, out_rgb = h * w * 3 bytes.  Not built: a stage per
 * slot or stream, a stage on input that is not raw Bayer, more than 8 bits between the demosaic and the matrix (a LINEAR 8-bit mosaic
 * followed by an sRGB curve has coarse shadows: the curve's first steps are several output levels apart).
 *
 * LENS SHADING of raw Bayer input, 8-, 10- and 12-bit alike: the gain that depends on the POSITION in the image (vignetting, the colour cast
 * towards the corners), which neither the position-blind raw table nor the per-pixel matrix can correct.  It comes FIRST: shading, raw
 * table, demosaic, colour stage; it maps a sample to a sample of the same depth.  `mesh` is uint16[4][mesh_h][mesh_w], phase-major as the
 * raw table, gains in Q12 (4096 is 1.0; any uint16 is legal), 2 <= mesh_w, mesh_h <= 64, node (0, 0) on pixel (0, 0) and node (mesh_h - 1,
 * mesh_w - 1) on pixel (img_h - 1, img_w - 1).  The gain of site (y, x), p its phase, in unsigned 32-bit integers:
 *     u = x * (mesh_w - 1) * 256 / (img_w - 1);  j = min(u >> 8, mesh_w - 2);  a = u - (j << 8)
 *     v = y * (mesh_h - 1) * 256 / (img_h - 1);  i = min(v >> 8, mesh_h - 2);  b = v - (i << 8)
 *     G = ((256-a)*(256-b)*mesh[p][i][j] + a*(256-b)*mesh[p][i][j+1] + (256-a)*b*mesh[p][i+1][j] + a*b*mesh[p][i+1][j+1] + 32768) >> 16
 * and a sample s (the byte, or the word masked to its bits) with the pedestal B = black[p], 0 <= B <= smax (255, or (1 << bits) - 1):
 *     s' = min(max(B + (((s - B) * G + 2048) >> 12), 0), smax)                       (int32, arithmetic shift: floor)
 * G = 4096 is the identity; the pedestal stays in place, so a raw table built with the same black level follows unchanged.  Everything a
 * context with a map computes from frames F is bit for bit what the same context without one computes from the frames taken through the two
 * lines above on the host (utils.apply_raw_shading).  lt_set_raw_shading(ctx, mesh, mesh_w, mesh_h, black, enable): enable != 0 sets the
 * map -- the mesh is expanded on the device into a gain plane uint16[img_h][img_w], allocated by the first set --, enable = 0 removes it and
 * frees the plane (no pointer is read); black = NULL is four zeros.  With a map set its kernels run whatever it holds, the identity
 * included; a set that fails on the device leaves the context WITHOUT a map, whatever it had.  Like lt_set_raw_color it waits for everything the context has in flight, governs what is launched afterwards, and is a set-up
 * or occasional call, NOT a per-frame one; raw table and colour stage may be set or changed before or after it.  LT_ERR_STATE in a context
 * whose input format is not raw Bayer, LT_ERR_INVALID for a mesh dimension outside 2 .. 64 or a black value outside 0 .. smax;
 * lt_set_input_format with another layout removes the map.  lt_get_raw_shading: *is_set := 0 / 1 and, where one is set, the mesh (4 *
 * mesh_w * mesh_h values; at most 4 * 64 * 64), its dimensions and the black values (any pointer may be NULL).  lt_get_raw_shading_plane:
 * the device's expanded plane, img_h * img_w values (LT_ERR_STATE without a map).  lt_raw_to_rgb_shaded is lt_raw_to_rgb_color behind a
 * map: the conversion alone, of one host frame in any of the twelve raw layouts; mesh = NULL is no map, and with ccm = curve = NULL there
 * is no colour stage either (the row kernels without one).  Not built: a map per stream or calibration set of a group, a map for input
 * that is not raw Bayer, meshes above 64 x 64, radial or polynomial models (sample them into a mesh on the host), a map change inside a
 * running stream. */
enum lt_input_layout { LT_INPUT_RGB = 0, LT_INPUT_NV12 = 1, LT_INPUT_I420 = 2, LT_INPUT_YUY2 = 3, LT_INPUT_UYVY = 4,
                       LT_INPUT_BGR = 5, LT_INPUT_RGBA = 6, LT_INPUT_BGRA = 7,
                       LT_INPUT_BAYER_RGGB = 16, LT_INPUT_BAYER_GRBG = 17, LT_INPUT_BAYER_GBRG = 18, LT_INPUT_BAYER_BGGR = 19,
                       LT_INPUT_BAYER10_RGGB = 32, LT_INPUT_BAYER10_GRBG = 33, LT_INPUT_BAYER10_GBRG = 34, LT_INPUT_BAYER10_BGGR = 35,
                       LT_INPUT_BAYER12_RGGB = 48, LT_INPUT_BAYER12_GRBG = 49, LT_INPUT_BAYER12_GBRG = 50, LT_INPUT_BAYER12_BGGR = 51,
                       LT_INPUT_BAYER10P_RGGB = 36, LT_INPUT_BAYER10P_GRBG = 37, LT_INPUT_BAYER10P_GBRG = 38, LT_INPUT_BAYER10P_BGGR = 39,
                       LT_INPUT_BAYER12P_RGGB = 52, LT_INPUT_BAYER12P_GRBG = 53, LT_INPUT_BAYER12P_GBRG = 54, LT_INPUT_BAYER12P_BGGR = 55 };
#define LT_YUV_BT601 {1220542, 1673527, -852492, -409993, 2116026}   /* video range; OpenCV's constants */
#define LT_YUV_BT709 {1220542, 1880097, -558891, -223347, 2214593}   /* video range */
int  lt_set_input_format(lt_ctx* ctx, int layout, const int32_t coeffs[5]);
int  lt_get_input_format(lt_ctx* ctx, int* layout, int32_t coeffs[5]);
int  lt_yuv_to_rgb(lt_ctx* ctx, const uint8_t* frame, int h, int w, int layout, const int32_t coeffs[5], uint8_t* out_rgb);
int  lt_bayer_to_rgb(lt_ctx* ctx, const uint8_t* frame, int h, int w, int layout, uint8_t* out_rgb);
int  lt_set_raw_lut(lt_ctx* ctx, const uint8_t* lut /* 1024 bytes, phase-major; NULL: none */);
int  lt_get_raw_lut(lt_ctx* ctx, uint8_t* lut /* 1024 bytes */, int* is_set);
int  lt_set_raw_lut_wide(lt_ctx* ctx, const uint8_t* lut /* 4 * entries bytes, phase-major; NULL: the default */, size_t entries);
int  lt_get_raw_lut_wide(lt_ctx* ctx, uint8_t* lut /* 4 * entries bytes */, size_t entries);
int  lt_raw16_to_rgb(lt_ctx* ctx, const uint16_t* frame, int h, int w, int layout, const uint8_t* lut /* 4 << bits bytes; NULL: the default */, uint8_t* out_rgb);
int  lt_set_raw_color(lt_ctx* ctx, const int16_t* ccm /* 9, row-major, Q10; NULL: identity */, const uint8_t* curve /* 256; NULL: identity */, int enable);
int  lt_get_raw_color(lt_ctx* ctx, int16_t* ccm /* 9 */, uint8_t* curve /* 256 */, int* is_set);
int  lt_raw_to_rgb_color(lt_ctx* ctx, const void* frame, int h, int w, int layout, const uint8_t* lut /* 4 * lut_entries bytes, or NULL */, size_t lut_entries,
                         const int16_t* ccm /* 9; NULL: identity */, const uint8_t* curve /* 256; NULL: identity */, uint8_t* out_rgb);
int  lt_set_raw_shading(lt_ctx* ctx, const uint16_t* mesh /* 4 * mesh_w * mesh_h, phase-major, Q12 */, int mesh_w, int mesh_h, const int32_t* black /* 4; NULL: zeros */, int enable);
int  lt_get_raw_shading(lt_ctx* ctx, uint16_t* mesh, int* mesh_w, int* mesh_h, int32_t* black /* 4 */, int* is_set);
int  lt_get_raw_shading_plane(lt_ctx* ctx, uint16_t* plane /* img_h * img_w */);

/* Raw sets: one raw table, colour stage and shading map per kind of camera, in ONE raw Bayer context -- held as calibration sets are.
 * Set 0 is the context's own: every function above acts on it.  lt_add_raw_set: a new set, a copy of set 0's value at that moment (its id
 * in *id; ids are bytes: at most 256 sets; LT_ERR_STATE in a context whose input format is not raw Bayer).  lt_set_input_format with
 * another layout removes every set but 0.  lt_set_slot_raw_sets: slot first_slot + i gets set ids[i] (LT_ERR_INVALID for an id the context
 * does not hold); cheap, a host table -- the launches carry the ids by value -- and a slot whose set changes has a stale front end.
 * lt_reserve, when it grows the context, puts every slot back to set 0.  The *_of functions are the setters and getters above for set `id`
 * (LT_ERR_INVALID for an id out of range): set-up or occasional calls behind everything in flight; the slots OF THAT SET get a stale front
 * end, no other.  lt_set_raw_lut_of / lt_get_raw_lut_of take the table of any raw layout, entries = 1 << bits per colour phase (256, 1024,
 * 4096; LT_ERR_INVALID for another count); NULL: none (8 bits) / the default (10, 12 bits); *is_set as lt_get_raw_lut's, 1 for 10 / 12 bits.
 * A front end or row conversion over slots that all have one set -- whichever -- launches the kernels of a context with that set alone; over
 * slots that mix sets it launches ONE set-per-slot kernel that runs the union of the parts the context's sets have, a set that lacks a part
 * running that part's exact identity (identity table, matrix 1024 I with identity curve, unit gains with pedestals 0): every slot's pixels
 * are those of a context with its set alone.  lt_raw_stats reads each slot's own map.  lt_last_raw_walk_form: which raw walks the front
 * end of the last lt_mask_run / lt_mask_rerun launched -- 0 none, 1 the one-set forms, 2 the set-per-slot forms (in some slice), -1 = no
 * run yet or a null context; tests use it to know which kernels they have exercised. */
int  lt_add_raw_set(lt_ctx* ctx, int* id);
int  lt_raw_set_count(lt_ctx* ctx, int* count);
int  lt_set_slot_raw_sets(lt_ctx* ctx, int first_slot, int n, const int32_t* ids);
int  lt_get_slot_raw_sets(lt_ctx* ctx, int first_slot, int n, int32_t* ids);
int  lt_set_raw_lut_of(lt_ctx* ctx, int id, const uint8_t* lut /* 4 * entries, phase-major; NULL */, size_t entries);
int  lt_get_raw_lut_of(lt_ctx* ctx, int id, uint8_t* lut, size_t entries, int* is_set);
int  lt_set_raw_color_of(lt_ctx* ctx, int id, const int16_t* ccm, const uint8_t* curve, int enable);
int  lt_get_raw_color_of(lt_ctx* ctx, int id, int16_t* ccm, uint8_t* curve, int* is_set);
int  lt_set_raw_shading_of(lt_ctx* ctx, int id, const uint16_t* mesh, int mesh_w, int mesh_h, const int32_t* black, int enable);
int  lt_get_raw_shading_of(lt_ctx* ctx, int id, uint16_t* mesh, int* mesh_w, int* mesh_h, int32_t* black, int* is_set);
int  lt_get_raw_shading_plane_of(lt_ctx* ctx, int id, uint16_t* plane /* img_h * img_w */);
int  lt_last_raw_walk_form(lt_ctx* ctx);
int  lt_raw_to_rgb_shaded(lt_ctx* ctx, const void* frame, int h, int w, int layout, const uint8_t* lut /* 4 * lut_entries bytes, or NULL */, size_t lut_entries,
                          const int16_t* ccm /* 9, or NULL */, const uint8_t* curve /* 256, or NULL */, const uint16_t* mesh /* or NULL: no map */, int mesh_w, int mesh_h,
                          const int32_t* black /* 4; NULL: zeros */, uint8_t* out_rgb);
/* Raw Bayer STATISTICS: the measuring half of the raw front end -- what an auto-exposure, black-level or auto-white-balance step between
 * windows reads before it builds the next raw table (lt_set_raw_lut / _wide).  lt_raw_stats takes them of what slots [first_slot, first_slot
 * + n) hold -- the attached surfaces where a slot has them, the slot's staging frame otherwise -- on the device, of the samples AS THEY ENTER
 * THE RAW TABLE: the byte (layouts 16 .. 19), the word masked to its low `bits` (32 .. 35, 48 .. 51), the unpacked sample (36 .. 39, 52 ..
 * 55), each taken through the shading map first where one is set (s' above).  Table, demosaic and colour stage play no part: white-balance
 * gains live in the table, so this is where a loop measures.  With p the phase of a site (0 R, 1 Gr, 2 Gb, 3 B, as the raw table's rows),
 * smax = 2^bits - 1 and bins = 256 / 1 << bits:
 *     rectangle   rows [row0, row1), columns [col0, col1), all even, inside the frame, not empty.  row1 == 0: the default rows -- the run
 *                 lt_get_input_rows names, which every upload entry point brings, rounded inward to even: (r0 + 1) & ~1, r1 & ~1 --;
 *                 col1 == 0: [0, img_w).  It is tiled by 2 x 2 cells anchored at even coordinates -- one site of each phase a cell --:
 *                 ncy = (row1 - row0) / 2 by ncx = (col1 - col0) / 2 cells.
 *     hist        uint32[n][4][bins]: hist[p][v] = the sites of phase p in the rectangle whose sample is v.  Every site counts.
 *     zones       a grid of grid_h x grid_w, 1 <= grid_h <= min(64, ncy), 1 <= grid_w <= min(64, ncx); cell (cy, cx), counted inside the
 *                 rectangle, lies in zone (cy * grid_h / ncy, cx * grid_w / ncx) (integer division).  A cell is VALID when all four of its
 *                 samples satisfy lo[p] <= s_p <= hi[p] (each bound 0 .. smax; lo > hi is legal: no valid cell).
 *     zone_count  uint32[n][grid_h][grid_w]: the valid cells of the zone.
 *     zone_sum    uint64[n][grid_h][grid_w][4]: the per-phase sums of the samples of the zone's valid cells.
 * Bit for bit utils.raw_stats (NumPy), whatever the order the device adds in: every quantity is an integer.  Any of the three outputs may
 * be NULL; rect, if not NULL, receives the rectangle used.  Like lt_set_raw_lut it waits for everything the context has in flight, runs on
 * the context's stream and the host waits for it: an occasional call, NOT a per-frame one.  Its device scratch is allocated by the first
 * call and freed with the context.  It changes nothing a later call reads: staging, camera frames, planes, records, lt_last_* answers and
 * attachments are as before.  LT_ERR_STATE in a context whose input format is not raw Bayer, and for a rectangle with rows outside the
 * default run while one of the slots holds only the rows the path reads (lt_upload_frame_rows without the rest; attached slots are whole);
 * LT_ERR_INVALID for NULL params, odd or out-of-frame bounds, a grid outside its limits, a bound outside 0 .. smax or a slot range outside
 * the capacity; n == 0 is LT_OK.  Not built: statistics behind the table or the demosaic, focus statistics, statistics inside a running
 * stream. */
typedef struct lt_raw_stats_params {
    int32_t row0, row1;      /* even; row1 == 0: the default rows */
    int32_t col0, col1;      /* even; col1 == 0: [0, img_w) */
    int32_t grid_h, grid_w;  /* 1 .. 64, at most the rectangle's cells per axis */
    int32_t lo[4], hi[4];    /* by phase, 0 .. smax */
} lt_raw_stats_params;
int  lt_raw_stats(lt_ctx* ctx, int first_slot, int n, const lt_raw_stats_params* p, uint32_t* hist /* n * 4 * bins, or NULL */,
                  uint32_t* zone_count /* n * grid_h * grid_w, or NULL */, uint64_t* zone_sum /* n * grid_h * grid_w * 4, or NULL */,
                  int32_t rect[4] /* out: row0, row1, col0, col1 used; may be NULL */);
/* Frames of another SIZE than the calibration's: a context with an input size of src_w x src_h takes RGB frames of src_h * src_w * 3
 * bytes and resizes them on the device to img_w x img_h -- cv2.resize(frame, (img_w, img_h)) with the default INTER_LINEAR, bit for bit:
 * half-pixel centres, 11-bit coefficients, OpenCV's two-stage rounding.  Everything the context computes, keeps and hands out is what a
 * plain context gives for the resized frames; annotated frames are img_w x img_h.  lt_set_input_size is called once, before the
 * context's first upload or attach, like lt_set_input_format: LT_ERR_INVALID for a width or height outside 1 .. 16384, LT_ERR_STATE
 * after an upload or in a context whose input format is not RGB (lt_set_input_format with a YUV layout on a context with an input size
 * is LT_ERR_STATE likewise); (img_w, img_h) clears the setting.  lt_get_input_size reads it back (the calibration's size without one).
 * In such a context every upload entry point below keeps its name and takes frames of the input size where it says frames_rgb.  Each
 * slot has a staging frame of the input size: the lt_upload_frame_rows family copies the source rows [s0, s1) that camera rows
 * [row0, row1) read -- lt_get_input_rows; lt_get_source_rows keeps its meaning, rows of the img_w x img_h frame -- and resizes
 * [row0, row1) into the slot's camera frame right behind the copy, ahead of whatever is launched over the slots next;
 * lt_upload_frames and the lt_upload_frame_rest family bring the source rows their rows read and leave the resized rows in the
 * camera frame (rows4 of lt_upload_frame_rest_rows are rows of the img_w x img_h frame).  The undistortion and everything behind
 * it read the camera frame as in a plain context.  lt_set_direct_upload returns 0 on such a context (its rows go to staging), and
 * lt_attach_device_frames returns LT_ERR_STATE: frames in device memory are not resized. */
int  lt_set_input_size(lt_ctx* ctx, int src_w, int src_h);
int  lt_get_input_size(lt_ctx* ctx, int* src_w, int* src_h);
int  lt_get_input_rows(lt_ctx* ctx, int* row0, int* row1);
/* frames: n * img_h * img_w * 3 bytes, RGB interleaved, as LaneTracker.process() receives them (:876) */
int  lt_upload_frames(lt_ctx* ctx, const uint8_t* frames_rgb, int first_slot, int n);
/* Camera rows [row0, row1) that undistort + warp actually read (a third of a 720-row frame at the reference
 * calibration).  lt_upload_frame_rows takes the same full-size host frames as lt_upload_frames but moves only
 * those rows: enough for lt_mask_run and the searches, not for lt_overlay_run, which shows the whole frame. */
int  lt_get_source_rows(lt_ctx* ctx, int* row0, int* row1);
int  lt_upload_frame_rows(lt_ctx* ctx, const uint8_t* frames_rgb, int first_slot, int n);
/* The same copy, waited for by nobody: enqueued on the slots' own streams -- behind everything launched over these slots so far
 * (and behind overlays of other streams that still read them), ahead of whatever is launched over them next -- and the call
 * returns (from pageable memory: once the runtime has the bytes on their way).  frames_rgb must stay valid and unchanged until a call that
 * waits for work launched over these slots afterwards has returned (lt_download_records of a search, lt_sync).  What
 * LaneTracker.process() uses (:876: one frame per call, the caller's array): the engine's copy runs under the mask chain's launches. */
int  lt_upload_frame_rows_enqueue(lt_ctx* ctx, const uint8_t* frames_rgb, int first_slot, int n);
/* A small lt_upload_frame_rows_enqueue (at most 1.5 MB of rows: the one 1280x720 frame of a process() call) does not go to the copy engine
 * where the device's memory is mapped into the process (large BAR): the calling thread stores the rows into the slot itself,
 * through the PCIe aperture -- 20 us of bus time for a 1280x720 frame's 914 KB instead of 22-24 us of call + 23 us of engine
 * copy + 6 us until the first kernel behind it.  The call then returns with the copy DONE (frames_rgb is the caller's again) after
 * waiting, on the host, for kernels that still read those slots' camera rows.  Same bytes, same results.
 * lt_set_direct_upload(ctx, on): 1 / 0 allows (the default) / forbids it, negative leaves the setting; returns 1 when such calls take
 * the aperture on this context, 0 when not (no large BAR, memory not mapped, forbidden; always 0 in a 4:2:0 context, whose rows
 * the engine copies into staging).  lt_direct_upload_count: calls that did. */
int  lt_set_direct_upload(lt_ctx* ctx, int on);
unsigned long long lt_direct_upload_count(lt_ctx* ctx);
/* The same rows without the host wait: the copy is enqueued on the context's copy stream behind the work already
 * enqueued for these slots, and everything enqueued for them afterwards waits for it -- the upload of one slot range
 * runs under the chain of the others (double-buffered host-fed pipeline).  frames_rgb must stay valid (and should be
 * page-locked, lt_host_alloc) until the next lt_sync. */
int  lt_upload_frame_rows_async(lt_ctx* ctx, const uint8_t* frames_rgb, int first_slot, int n);
/* The complement: every other row of the same frames, enqueued on a copy stream of its own so that it runs beside
 * the mask chain (call it after lt_mask_run).  The host buffer must stay valid until the next lt_sync or download;
 * lt_overlay_run waits for it. */
int  lt_upload_frame_rest(lt_ctx* ctx, const uint8_t* frames_rgb, int first_slot, int n);
/* Of that complement, only the rows inside the two runs rows4 = {a0, a1, b0, b1} (NULL: all of it, as above): what
 * lt_present_frame with the same runs reads.  The other rows of the slots keep whatever they held -- an overlay over the whole
 * frame needs lt_upload_frame_rest first. */
int  lt_upload_frame_rest_rows(lt_ctx* ctx, const uint8_t* frames_rgb, int first_slot, int n, const int32_t* rows4);
/* The pointer-list forms of lt_upload_frame_rows_enqueue and lt_upload_frame_rest: frame k comes from its own host array
 * frames_rgb[k] (img_h * img_w * 3 bytes) and goes into slot first_slot + k -- the camera frames of n unrelated streams, one
 * each, without gathering them into one block on the host first.  Slot by slot they are the range forms' calls: the same rows,
 * the same ways (a frame's rows may take the PCIe aperture, lt_set_direct_upload), the same ordering against the slots' readers
 * and writers, and frames_rgb[k] must stay valid as long as the range form's frames_rgb.  The list itself is read before the
 * call returns. */
int  lt_upload_frame_rows_list(lt_ctx* ctx, const uint8_t* const* frames_rgb, int first_slot, int n);
int  lt_upload_frame_rest_list(lt_ctx* ctx, const uint8_t* const* frames_rgb, int first_slot, int n);
/* ---- camera frames that are already in device memory --------------------------------------------------------------------------
 * A decoder or a capture pipeline hands its surfaces out in device memory, usually with a row pitch above the width and the
 * chroma plane somewhere else.  Such frames are not copied: the undistortion -- the only kernel that reads camera pixels on the
 * way to a lane record -- fetches its taps from the surfaces themselves.  One lt_device_surface per frame, in the layout of the
 * context's input format: plane[0] the RGB rows (3 bytes a pixel) or the Y plane, `pitch` bytes from row to row; NV12: plane[1]
 * the rows of (U, V) pairs; I420: plane[1] the U and plane[2] the V plane; `chroma_pitch` bytes between chroma rows.  YUY2 / UYVY:
 * plane[0] the one plane, `pitch` >= 2 * img_w; BGR: >= 3 * img_w; RGBA / BGRA: >= 4 * img_w; chroma_pitch is not read.  Any byte
 * alignment of pointers and pitches is taken (a column crop of an RGB frame starts at 3 * x0).  Results are bit for bit those of
 * the same bytes uploaded from the host.
 *
 * lt_attach_device_frames: from now on the front end of slots [first_slot, first_slot + n) reads surfaces[0 .. n).  Ordered like
 * lt_upload_frame_rows_enqueue -- behind everything launched over these slots so far, ahead of whatever is launched over them
 * next -- and with its contract for the caller's memory: the surfaces hold their final content when the call is made (wait for
 * the producer first) and stay valid and unchanged until a call that waits for work launched over these slots afterwards has
 * returned (lt_download_records of a search, lt_sync).  The list itself is read before the call returns.  Any lt_upload_* of
 * camera rows into a slot detaches it; lt_mask_run takes ranges that mix attached and plain slots, lt_mask_rerun reuses the
 * front end of an attached slot like any other.
 * Every plane is checked on the host BEFORE anything is launched: device memory of the context's device, known to the HIP
 * runtime this library is linked against, its whole extent -- pitch * (rows - 1) + row bytes -- inside one allocation; pitches at
 * least a row wide and below 2^23.  Anything else is LT_ERR_INVALID with a message, nothing is launched and the context is as it
 * was.  (A pointer of another runtime in the same process -- a framework that bundles its own copy of the HIP runtime -- is
 * unknown to this one and refused.)  The verdict is not remembered: every call checks again.
 *
 * lt_device_frames_rest: the counterpart of lt_upload_frame_rest / _rest_rows for attached slots -- the rows a SHOWN frame needs
 * (rows4 = {a0, a1, b0, b1}: those two runs, whole; NULL: the whole frame) are brought from the surfaces into the slots' RGB
 * camera frames on the device, converted where the context is 4:2:0, on the copy stream beside the mask chain; lt_overlay_run
 * waits for it.  LT_ERR_STATE for a slot that is not attached.  A search-only caller never needs it: nothing is copied then. */
typedef struct lt_device_surface {
    const void* plane[3];
    int32_t pitch;               /* bytes between rows of plane[0] */
    int32_t chroma_pitch;        /* bytes between rows of plane[1] (and plane[2]); not read in an RGB or a 4:2:2 context */
} lt_device_surface;
int  lt_attach_device_frames(lt_ctx* ctx, const lt_device_surface* surfaces, int first_slot, int n);
int  lt_device_frames_rest(lt_ctx* ctx, int first_slot, int n, const int32_t* rows4);
/* ---- calibration sets: one context, cameras of different calibrations ------------------------------------------------------------
 * A context holds one or more calibration SETS -- the remap tables of one camera: its intrinsics, its distortion, its bird's-eye
 * homography -- and every slot has one of them.  Set 0 is the calibration lt_create was given, and every slot starts with it: a
 * context that never adds a set is what it always was, launch for launch.
 *
 * lt_add_calibration: a further set from `calib`; *id is its number (1, 2, ...; at most 256 sets).  img_w, img_h, warp_w and warp_h
 * must equal the context's (LT_ERR_INVALID).  Like lt_set_input_format it belongs in front of the context's first upload or
 * attach: LT_ERR_STATE afterwards.  The GEOMETRY stays one per context: the rows of the undistorted image the front end fills, the
 * camera rows the uploads bring (lt_get_source_rows) and the rows a lane can reach (lt_overlay_rows) become the UNIONS over the
 * sets of what each set needs, and every set's undistortion table is built for that union.  Rows a set's own warp never
 * references are computed and never read: a slot's planes, mask and record are bit for bit those of a context created with its
 * set alone.  (lt_get_info's src_row0 / src_row1 and lt_download_undistorted follow the union.)
 * lt_calibration_count: the sets the context holds, set 0 included.
 * lt_set_slot_calibrations: slot first_slot + i gets set ids[i] (LT_ERR_INVALID for an id the context does not hold).  Cheap -- a
 * host table; the launches carry the ids by value, so nothing has to be ordered on the device and an assignment may change every
 * tick.  A slot whose set changes has a stale front end: lt_mask_rerun over it runs the front end again.  lt_reserve, when it
 * grows the context, puts every slot back to set 0.  lt_get_slot_calibrations reads the assignment back.
 * lt_overlay_configure_set: lt_overlay_configure for one set (lt_overlay_configure is set 0's).
 *
 * lt_mask_run / lt_mask_rerun over slots of ONE set -- whichever -- launch the kernels they always launched, with that set's tables;
 * a stream slice that MIXES sets takes table-per-slot forms of the undistortion and of the warp (one launch each, whatever the
 * number of sets; frames in slots or attached, RGB / NV12 / I420).  lt_overlay_run / lt_overlay_run_rows draw every slot through
 * the inverse-warp table of its own set (LT_ERR_STATE if that set's overlay is not configured), run by run over consecutive
 * slots of one set; lt_overlay_text and the downloads do not depend on the set; lt_download_bev warps every slot with its own.
 * Everything else that reads calibration tables knows set 0 only and REFUSES a slot that has another set with LT_ERR_STATE,
 * nothing launched and the context as it was: lt_present_frame, lt_present_lane_async, lt_present_lane_from_fit_async,
 * lt_present_finish, lt_overlay_run_strip, lt_overlay_run_strip_coeffs, lt_search_viz_run, lt_split_panes_run -- and
 * lt_lane_spans_from_fit, which names no slot, while ANY slot of the context has another set. */
int  lt_add_calibration(lt_ctx* ctx, const lt_calib* calib, int* id);
int  lt_calibration_count(lt_ctx* ctx, int* count);
int  lt_set_slot_calibrations(lt_ctx* ctx, int first_slot, int n, const int32_t* ids);
int  lt_get_slot_calibrations(lt_ctx* ctx, int first_slot, int n, int32_t* ids);
int  lt_overlay_configure_set(lt_ctx* ctx, int set, const double* Minv /* 9 */);
/* Device blocks out of the library's own cache (lt_device_cache_stats counts them as live), with plain synchronous copies
 * from and to host memory: for callers that have no HIP binding of their own -- the Python package, tools, tests -- and want to
 * hold frames on the device in the runtime the library lives in.  lt_device_write / lt_device_read refuse ranges that do not lie
 * inside such a block; lt_device_free waits for the device first, as hipFree does. */
int  lt_device_alloc(int device, size_t bytes, void** out);
int  lt_device_free(void* block);
int  lt_device_write(void* dst_device, const void* src_host, size_t bytes);
int  lt_device_read(void* dst_host, const void* src_device, size_t bytes);
/* The host waits for a producer's stream of this runtime before its frames are attached: 1 the legacy default stream, 2 the
 * per-thread default stream (the numbers of __cuda_array_interface__), anything else a hipStream_t; 0 is LT_ERR_INVALID. */
int  lt_device_stream_wait(int device, uintptr_t stream);
/* masks: n * warp_h * warp_w bytes; lets the search stages run on caller-supplied binary images */
int  lt_upload_masks(lt_ctx* ctx, const uint8_t* masks, int first_slot, int n);
/* The same as bit planes, an eighth of the bytes: n * warp_h * wpr 64-bit words, wpr = (warp_w + 63) / 64, dense; pixel x of a row is
 * bit x % 64 of the row's word x / 64, least significant bit first.  A set bit is a mask byte != 0: lt_download_masks gives 255
 * for it.  Bits at columns >= warp_w need not be zero: the library clears them on the way in.  Slots filled this way are searched
 * by the bit-plane kernels wherever those take the geometry (as behind lt_mask_run; lt_last_search_source tells), slots filled by
 * lt_upload_masks by the u8 kernels.  The u8 kernels sum byte values where the bit-plane kernels count pixels; the sums are only
 * compared and maximised, so both give the same lane pixels, centroids and fits for every mask whose non-zero bytes are all equal. */
int  lt_upload_mask_bits(lt_ctx* ctx, const uint64_t* bits, int first_slot, int n);
int  lt_download_masks(lt_ctx* ctx, int first_slot, int n, uint8_t* masks);
int  lt_download_plane(lt_ctx* ctx, int plane, int first_slot, int n, uint8_t* out);
/* the undistorted camera rows [src_row0, src_row1) as RGB interleaved: n * rows * img_w * 3 */
int  lt_download_undistorted(lt_ctx* ctx, int first_slot, int n, uint8_t* out);
int  lt_download_records(lt_ctx* ctx, int first_slot, int n, lt_lane_record* out);
/* side 0 = left, 1 = right.  Writes at most cap (y,x) pairs in reference order; returns the count
 * through *count (self.left_y/left_x/right_y/right_x, :434-437, :492-495). */
int  lt_download_pixels(lt_ctx* ctx, int slot, int side, int32_t* ys, int32_t* xs, int cap, int* count);
/* self.left_window_centroids / right_window_centroids (:439-440) */
int  lt_download_centroids(lt_ctx* ctx, int slot, int side, int32_t* out, int cap, int* count);
/* Both sides' lane pixels and, with want_centroids, both window-centroid lists of a slot in ONE round trip to the device (the lists
 * of lane_tracker.py:434-440 / :492-495 as lt_download_pixels and lt_download_centroids return them).  counts[2] / cent_counts[2]:
 * the full lengths (left, right); lists longer than cap / cent_cap are cut.  LT_ERR_CAPACITY when the slot's list region does not
 * fit the staging buffer (very large search windows): use the two calls above. */
int  lt_download_lane_lists(lt_ctx* ctx, int slot, int32_t* left_y, int32_t* left_x, int32_t* right_y, int32_t* right_x, int cap, int* counts,
                            int want_centroids, int32_t* cent_left, int32_t* cent_right, int cent_cap, int* cent_counts);
/* device-to-device copy of n records into caller-owned device memory (e.g. a collective's send buffer) */
int  lt_copy_records_to_device(lt_ctx* ctx, int first_slot, int n, void* dst_device);
/* the same copy enqueued behind the slots' searches on the context's streams, without waiting: the records are in
 * dst_device after the next lt_sync (several steps can fill one send buffer and be gathered once) */
int  lt_enqueue_records_to_device(lt_ctx* ctx, int first_slot, int n, void* dst_device);

/* ---- the hot path, device resident ----------------------------------------------------------- */
/* find_lane_points() part 1 (:832-846): undistort -> warpPerspective -> filter_lane_points. */
int  lt_mask_run(lt_ctx* ctx, int first_slot, int n, const lt_filter_params* p);
/* The same over slots whose frames have been through lt_mask_run already, with OTHER filter parameters -- the second try of a frame
 * (lane_tracker.py:1081-1101: the 'neighborhood' set over the same bird's-eye image): the undistortion and the warp are skipped
 * where a slot's R / Lab-b planes are still those of the frame it holds (any upload of camera rows into the slot, or lt_filter_run,
 * ends that), and run as in lt_mask_run where they are not.  Results are those of lt_mask_run. */
int  lt_mask_rerun(lt_ctx* ctx, int first_slot, int n, const lt_filter_params* p);
/* filter_lane_points() only, on bird's-eye RGB images already uploaded with lt_upload_bev (:183-240) */
int  lt_upload_bev(lt_ctx* ctx, const uint8_t* bev_rgb, int first_slot, int n);
int  lt_filter_run(lt_ctx* ctx, int first_slot, int n, const lt_filter_params* p);
/* The fit of every search below (and of lt_fit_poly2): integer moments, moved exactly to the pixels' own mean row, 3 x 3 Cholesky in
 * f64 -- within the BASELINE tolerance (1e-4 relative) of exact rational least squares for a dash of three adjacent rows at the image's
 * edge as for a full-height lane of 16384 rows (sum dy^4 is kept in 128 bits).  fit_flags bit 0 / 1: the left / right lane has
 * fewer than 3 distinct rows, its coefficients are 0.
 * Size limits, refused with LT_ERR_INVALID before anything is launched: a search that only the first-formulation kernels take
 * keeps its row counters in LDS, 150 KB at most -- a band search with bandwidth > 31 (a band wider than 64 columns), a width that
 * is no multiple of 4 or more than 4795 band rows, and any band search on an image taller than 8192 rows: at most 9590 image rows;
 * a sliding-window search outside k_sws_fit2's geometry: 16 * window_height + 8 * width bytes.  Likewise a sliding window wider
 * than the image (2 * int(window_width / 2) > warp_w): the reference's window slice then wraps round the image edge and yields
 * negative columns. */
/* sliding_window_search() + fit_poly() (:242-447, :502-509) on the slots' masks */
int  lt_sws_fit_run(lt_ctx* ctx, int first_slot, int n, const lt_search_params* p);
/* band_search() + fit_poly() (:449-509); prev_coeffs: n * 6 doubles (last_left_coeffs, last_right_coeffs) */
int  lt_band_fit_run(lt_ctx* ctx, int first_slot, int n, const lt_search_params* p, const double* prev_coeffs);
/* The searches of n frames of UNRELATED streams, each in its own mode, in one launch: items[i] names the slot, the mode (0:
 * sliding_window_search with `sws`, 1: band_search with `band` around items[i].prev_coeffs) -- every slot holds what
 * lt_sws_fit_run / lt_band_fit_run over that slot alone would leave there: record, lane pixels and (sliding window) window
 * centroids.  The slots need not be contiguous or in order; each may appear once.  sws / band may be NULL when no item has
 * that mode.  Frames whose geometry the one-launch kernel does not take (a window wider than 64 columns, a band wider than
 * 64, masks without bit planes) are searched slot by slot with the kernels of the range forms -- same results.  Enqueued behind
 * the work on every listed slot (every slot stream holding one waits for the search before its later work); `items` is read
 * before the call returns.  The context stages one list at a time: a call first waits, on the host, until the searches of the
 * previous list call have finished reading theirs (nothing to wait for when its records have been downloaded).  LT_ERR_INVALID: n < 0, a NULL list or parameter set that is needed, a slot outside the capacity or
 * listed twice, a mode other than 0 / 1. */
int  lt_search_fit_list(lt_ctx* ctx, int n, const lt_search_item* items, const lt_search_params* sws, const lt_search_params* band);
/* The warm path of ONE stateful stream, chained on the device (band_search :449-500 + fit_poly :502-509 per frame, with
 * the cross-frame dependence of :474-489 / :1182-1183 kept in HBM): the slots first_slot .. first_slot + n - 1 hold
 * consecutive frames of one video; the band of the first is drawn around seed_coeffs (6 doubles: last_left_coeffs,
 * last_right_coeffs) or, if seed_coeffs is NULL, around the fit in the record of slot first_slot - 1; the band of every
 * later frame around the fit of the frame before it -- what the reference does as long as every frame is found valid.
 * Validity (check_validity, :561-627) stays on the host: the caller collects the n records once, keeps those up to the
 * first frame it rejects and discards the rest (speculation; results never differ from the frame-by-frame calls).  The
 * walk stops by itself behind a frame without both lanes or with a rank-deficient fit; the slots it did not search get
 * detected = 0 and mode = 255.  LT_ERR_STATE if 2 * bandwidth + 2 > 64 or the mask width is not a multiple of 4
 * (use lt_band_fit_run frame by frame then).
 * The chain is one workgroup: it runs on a stream of its own behind the work already enqueued for its slots, beside the
 * mask chains of later slots, and leaves its records (with a NULL seed also the seed record of slot first_slot - 1) in
 * page-locked host memory.  lt_band_fit_chain_collect copies records [first_slot, first_slot + n) of the most recent
 * chain covering that range to `out`, waiting for that chain only -- not for the device; every lt_download_* / lt_sync
 * also waits for all chains. */
int  lt_band_fit_chain_run(lt_ctx* ctx, int first_slot, int n, const lt_search_params* p, const double* seed_coeffs);
int  lt_band_fit_chain_collect(lt_ctx* ctx, int first_slot, int n, lt_lane_record* out);
/* Give the chained search n CUs of its own (0 = none, the default): the context's compute streams are recreated with a CU
 * mask that keeps them off CUs 0 .. n-1, and the search stream is restricted to those.  Why: the kernels of the mask chain
 * spread their workgroups over the chip once, statically; a workgroup of the chain kernel sharing ONE CU with them slows that
 * CU's share of every mask kernel, and each kernel then ends with that CU -- measured: the mask chain of 128-frame launches
 * takes 18.6 us per frame beside a running chain, 15.1 with one CU set aside (12.8 alone).  With n >= 2 the search has CU 0
 * and the others belong to the download stream (used when LT_DL_KERNEL=1 copies annotated frames back with a kernel).  Call it
 * on an idle context (it synchronises); a context that only processes independent batches has no use for it. */
int  lt_set_search_cus(lt_ctx* ctx, int n);
/* The bilateral threshold (lane_tracker.py:14-83, :214-215) has two kernels: walks down half rows / columns with running sums
 * (k_bilateral_walk_hv), which win once a call brings enough frames to fill the chip, and 128 x 128 tiles in LDS
 * (k_bilateral_tile2) for the few frames of a process() call or a short chunk.  A call of at least `frames` frames (of this
 * context's bird's-eye size) takes the walks; default: 80 frames' worth of 1100 x 1080 pixels, the crossover measured on MI355X
 * (64 frames: 232 vs 210 us, 96 frames: 255 vs 304 us).  0: always walk; negative: the default again.  Results never depend on it. */
int  lt_set_walk_min_frames(lt_ctx* ctx, int frames);
/* Urgent mode, for the frame of a stateful stream whose first try failed (lane_tracker.py:1071-1128: second parameter set,
 * second search) while masks of later frames are already queued: between lt_set_urgent(ctx, 1) and lt_set_urgent(ctx, 0),
 * lt_mask_run / lt_filter_run / lt_sws_fit_run / lt_band_fit_run run on a stream of their own, behind the work enqueued for
 * THEIR slots only, and the lt_download_* calls wait for that stream only (they must ask for results produced in urgent mode,
 * or already complete).  Work enqueued for those slots afterwards is ordered behind it.  Leaving the mode waits for it. */
int  lt_set_urgent(lt_ctx* ctx, int on);
/* The caller has rejected a frame: every chain enqueued so far ON THIS CONTEXT -- whatever its slot range -- stops at its
 * next frame (the slots it has not searched get mode 255) instead of finishing its speculation.  Chains enqueued
 * afterwards are not affected.  One context serves one stream; independent streams take separate contexts. */
int  lt_band_fit_chain_cancel(lt_ctx* ctx);
/* tag records with global frame indices first_frame, first_frame+1, ... */
int  lt_set_frame_base(lt_ctx* ctx, int first_slot, int n, int first_frame);

/* ---- host-buffer convenience wrappers (upload + run + download) -------------------------------- */
int  lt_mask_batch(lt_ctx* ctx, const uint8_t* frames_rgb, int n, const lt_filter_params* p, uint8_t* masks);
/* masks == NULL: use the device-resident masks of slots [0,n) */
int  lt_sws_fit_batch(lt_ctx* ctx, const uint8_t* masks, int n, const lt_search_params* p, lt_lane_record* out);
int  lt_band_fit_batch(lt_ctx* ctx, const uint8_t* masks, int n, const lt_search_params* p,
                       const double* prev_coeffs, lt_lane_record* out);

/* ---- single-image operators with the reference's module-level signatures ----------------------- */
/* bilateral_adaptive_threshold(img, ksize, C, mode, true_value, false_value) (:14-83).
 * mode 0 'floor', 1 'ceil', anything else -> LT_ERR_INVALID (the reference's ValueError, :71). */
int  lt_bilateral_adaptive_threshold(lt_ctx* ctx, const uint8_t* img, int h, int w, int ksize, int C,
                                     int mode, int true_value, int false_value, uint8_t* out);
/* LaneTracker.filter_lane_points(img, ...) on one bird's-eye RGB image of any size (:183-240) */
int  lt_filter_lane_points(lt_ctx* ctx, const uint8_t* bev_rgb, int h, int w, const lt_filter_params* p,
                           uint8_t* mask);

/* One elliptical morphology operator on a single-channel image of any size: the building block of
 * morphologyEx (:210-211, :238).  k in {5, 29, 55}; op 0 erode, 1 dilate, 2 top-hat, 3 open.
 * direct != 0 evaluates the footprint tap by tap instead of using the run decomposition (k = 5 always does). */
int  lt_morph_ellipse(lt_ctx* ctx, const uint8_t* img, int h, int w, int k, int op, int direct, uint8_t* out);
/* Test hook: ONE call of the top-hat launchers on n dense h x w planes given by value, in buffers that live for this call only
 * (source, intermediate, destination, copy plane, and the split-band form's zone scratch when n > 2, sized as the mask chain sizes it).
 *   k       29 or 55
 *   op      0 erode, 1 dilate, 2 top-hat (src - dilate(erode(src))), 3 top-hat that also stores its minuend into the copy plane
 *   bands   0: the launcher's own rule; > 0: that many bands (k_morph_one and k_morph_one_pair keep even bands of at least 8 rows)
 *   dpitch  0: a dense destination; otherwise (w + 63) & ~63, the pitch of the planes the threshold walks read (the last launch only)
 *   route   0: launch_morph_runs; 1: launch_morph_one_pair on 2 n planes -- n for the 55x55 chain, then n for the 29x29 chain, n <= 2,
 *           op 0 .. 2, k ignored beyond its check -- whose refusal of a geometry comes back as *launched = 0 (nothing ran)
 * dst_out, mid_out (the eroded intermediate; required for op >= 2, dense) and copy_out (required for op 3) receive the WHOLE allocations:
 * n + 2 planes per chain (route 1: the 55x55 chain's n + 2, then the 29x29 chain's), rows of dpitch bytes where dpitch != 0, every byte
 * 0xA5 before the launch, the work in planes 1 .. n.  Whatever is not 0xA5 in planes 0 and n + 1 or in columns [w, dpitch) was stored
 * out of place.  *report: what ran (the last launch of the call). */
typedef struct lt_morph_report {
    int32_t family;        /* 0 nothing, 1 k_morph_one, 2 k_morph_one_pair, 3 k_morph_runs2 (bands walk their halos), 4 k_morph_split, 5 k_morph_runs (one row) */
    int32_t wide;          /* 1: rows moved as dwords; 0: the narrow (byte) form */
    int32_t nbands, band_rows;
    int32_t pair_strip;    /* 1: the last strip carries two frames per wave */
    int32_t q;             /* waves per task of families 1 and 2, else 0 */
    int32_t nbands29, band_rows29;   /* family 2: the 29x29 plane's cut (nbands / band_rows are the 55x55 plane's) */
} lt_morph_report;
int  lt_morph_planes(lt_ctx* ctx, const uint8_t* planes, int n, int h, int w, int k, int op, int bands, int dpitch, int route,
                     uint8_t* dst_out, uint8_t* mid_out, uint8_t* copy_out, lt_morph_report* report, int* launched);
/* cv2.resize(img, (dw, dh)) with the default INTER_LINEAR on a u8 image of 1 or 3 interleaved channels (host memory in and
 * out): half-pixel centres, 11-bit coefficients, OpenCV's two-stage fixed-point rounding. */
int  lt_resize_linear_u8(lt_ctx* ctx, const uint8_t* img, int h, int w, int channels, int dh, int dw, uint8_t* out);

/* LaneTracker.fit_poly() on explicit pixel lists (np.polyfit(ys, xs, 2), :506-507): n (y,x) pairs with
 * coordinates in [0, 65535], for any h, w >= 1: they only name the point the moments are taken about, (h / 2, w / 2) kept inside
 * [0, 65535]; the sums that can pass 64 bits are kept in 128, so any list an int counts is solved.  *rank_deficient is set when
 * fewer than 3 distinct y exist (coef = 0). */
int  lt_fit_poly2(lt_ctx* ctx, const int32_t* ys, const int32_t* xs, int n, int h, int w, double coef[3],
                  int* rank_deficient);

/* ---- presentation stage (next row after the hot path) ------------------------ */
/* Minv: the pickled inverse perspective matrix the reference hands to warpPerspective in draw_lane
 * (lane_tracker.py:648); builds the camera-sized remap table once.  Call it BEFORE uploading frames whose annotated form will be
 * asked for: when the rows the lane can reach (lt_overlay_rows) stick out of the rows lt_upload_frame_rows brings by a few rows
 * (458-696 against 457-695 of 720 with the reference calibration), that run is widened to cover them (lt_get_source_rows reports
 * the new run), so that an annotated frame's lane rows need no upload of their own; a frame uploaded before lacks those rows.
 * The run only ever widens: another lt_overlay_configure, or a further calibration set, never takes rows away. */
int  lt_overlay_configure(lt_ctx* ctx, const double* Minv /* 9 */);
/* draw_lane() without the text (lane_tracker.py:637-662) for the frames in slots [first, first+n):
 * fillPoly of the polygon left points + reversed right points in (0,255,0), warpPerspective with Minv,
 * addWeighted(frame, 1, lane, alpha, 0).  left_n/right_n: points per slot; left_yx/right_yx: (y, x)
 * int32 pairs of all slots, concatenated.  A slot with no points yields a copy of its frame. */
int  lt_overlay_run(lt_ctx* ctx, int first_slot, int n, const int32_t* left_n, const int32_t* right_n,
                    const int32_t* left_yx, const int32_t* right_yx, double alpha);
/* The same, drawing only two runs of camera rows rows4 = {a0, a1, b0, b1} of every frame (NULL: whole frames): for annotated
 * frames that travel back as row runs (lt_download_overlay_rows_async; lt_overlay_rows says which rows the lane can reach). */
int  lt_overlay_run_rows(lt_ctx* ctx, int first_slot, int n, const int32_t* left_n, const int32_t* right_n,
                         const int32_t* left_yx, const int32_t* right_yx, double alpha, const int32_t* rows4);
/* Text on the annotated frames (putText in draw_lane / print_failure, :653-672).  OpenCV's Hershey glyphs are
 * not reproduced: the caller supplies its own glyph atlas once -- n_glyphs alpha cells of glyph_w x glyph_h bytes
 * for the characters first_char, first_char + 1, ..., and each character's advance width (<= glyph_w). */
int  lt_overlay_set_font(lt_ctx* ctx, const uint8_t* atlas, const uint8_t* advance, int first_char, int n_glyphs,
                         int glyph_w, int glyph_h);
/* Blend n_lines white text lines into the annotated frame of every slot in [first, first+n) (after lt_overlay_run).
 * lines: n * n_lines * line_len bytes, zero-padded; line i of a slot starts at (x0, y0 + i * step). */
int  lt_overlay_text(lt_ctx* ctx, int first_slot, int n, const char* lines, int n_lines, int line_len, int x0, int y0,
                     int step);
/* The camera rows [*row0, *row1) in which draw_lane()'s inverse warp (lane_tracker.py:648) can place a lane pixel at all, from
 * the table lt_overlay_configure built: every pixel of an annotated frame outside these rows and outside the text lines equals
 * the camera pixel, whatever the polygon. */
int  lt_overlay_rows(lt_ctx* ctx, int* row0, int* row1);
/* draw_lane() / print_failure() (lane_tracker.py:629-673) for ONE resident frame in one call: lt_overlay_run with one polygon
 * (left_n / right_n: one count each), lt_overlay_text when lines != NULL, and the annotated frame into `out` (img_h * img_w * 3
 * bytes, page-locked memory preferred); returns when it is there.  rows4 = NULL: the whole frame.  rows4 = {a0, a1, b0, b1},
 * two ordered runs of camera rows: only these rows are drawn and written, at their places in `out` -- the caller fills the
 * others from the camera frame it holds (LaneTracker.process() does so while the device is busy, and half the frame crosses the
 * bus).  The runs must cover the text lines and, for a non-empty polygon, lt_overlay_rows; LT_ERR_INVALID otherwise. */
int  lt_present_frame(lt_ctx* ctx, int slot, const int32_t* left_n, const int32_t* right_n, const int32_t* left_yx,
                      const int32_t* right_yx, double alpha, const char* lines, int n_lines, int line_len, int x0, int y0,
                      int step, uint8_t* out, const int32_t* rows4);
/* lt_present_frame in two halves, for a caller that knows the polygon before it knows the text (radius, eccentricity and the
 * verdict on the frame take LaneTracker.process() another 25 us of host work behind the record).  lt_present_lane_async draws
 * both row runs (rows4 is required: the text lines in the first run, lt_overlay_rows in the second, the two apart) and sends the
 * second run on its way without waiting; lt_present_finish blends the text into the first run, sends it and waits for both.  A
 * first half that turns out to be for nothing (the frame was invalid) is followed by a whole lt_present_frame on the same slot
 * and `out`, which draws and sends everything again. */
int  lt_present_lane_async(lt_ctx* ctx, int slot, const int32_t* left_n, const int32_t* right_n, const int32_t* left_yx,
                           const int32_t* right_yx, double alpha, uint8_t* out, const int32_t* rows4);
int  lt_present_finish(lt_ctx* ctx, int slot, const char* lines, int n_lines, int line_len, int x0, int y0, int step,
                       uint8_t* out, const int32_t* rows4);
/* The first half without the host: the averaged lane of the frame in `slot` (draw_lane's polygon, :629-662, of the running average
 * :1182-1189 that this frame's fit would give) drawn by the device itself, enqueued on the slot's stream right behind its search --
 * call it after lt_band_fit_run / lt_sws_fit_run over that one slot, before waiting for the record.  prev_sum: the sum, in order,
 * of the older fits (left a, b, c, right a, b, c) that stay in the average, count: fits in the average with this frame's (1: this
 * frame's alone, prev_sum ignored); ploty / ploty2: get_poly_points' rows and their squares (:514).  One workgroup forms average,
 * plot points and the polygon's row intervals from the fit in the slot's record with the host's f64 operations in the host's order;
 * the overlay stores the rows of rows4's second run (its first run must be empty: text on the host) into the page-locked `out`.
 * A record without a usable fit (nothing detected, fit_flags != 0) draws nothing; lt_present_finish waits for the rows.  Returns
 * LT_ERR_STATE where this form does not exist (out not page-locked / 16-byte aligned, too many plot rows): draw with
 * lt_present_lane_async then.  lt_lane_spans_from_fit: the same workgroup for a fit given by value, its row intervals
 * (warp_h x (lo, hi) int16) brought back -- for tests. */
int  lt_present_lane_from_fit_async(lt_ctx* ctx, int slot, const double* prev_sum, int count, const double* ploty,
                                    const double* ploty2, int n_rows, double alpha, uint8_t* out, const int32_t* rows4);
int  lt_lane_spans_from_fit(lt_ctx* ctx, const double* fit6, int detected, int fit_flags, const double* prev_sum, int count,
                            const double* ploty, const double* ploty2, int n_rows, int16_t* spans_out);
/* Host-only helper (no GPU needed): the (lo, hi) column interval per bird's-eye row that cv2.fillPoly
 * paints for that polygon; empty rows are (32767, -32768).  spans: warp_h * 2 int16. */
int  lt_lane_polygon_spans(int warp_h, const int32_t* left_yx, int n_left, const int32_t* right_yx, int n_right,
                           int16_t* spans);
/* Host-only helper (no GPU needed): get_poly_points (lane_tracker.py:511-528) for n pairs of parabolas, in the packed form
 * lt_overlay_run takes.  coeffs: n * 6 doubles (left a, b, c, right a, b, c); ploty / ploty2: the n_rows plot rows and their
 * squares, as the caller's NumPy computed them.  fitx = a * ploty2 + b * ploty + c in exactly these IEEE operations; points
 * with 0 <= fitx <= warp_w - 1 are kept, x truncated, y = warp_h - count .. warp_h - 1 (upstream's rule).  left_n / right_n:
 * n counts; left_yx / right_yx: room for n * n_rows (y, x) pairs each, written back to back. */
int  lt_poly_points(int warp_w, int warp_h, const double* coeffs, int n, const double* ploty, const double* ploty2, int n_rows,
                    int32_t* left_n, int32_t* right_n, int32_t* left_yx, int32_t* right_yx);
/* Host-only (no GPU needed): what LaneTracker.process() computes between a frame's record and its text lines when the frame's first
 * try is valid -- check_validity (:561-627), the running average of the fits (:1186-1187), get_poly_points of the averaged curves
 * (:511-528), get_curve_radius through the pixel fit (:530-549) and get_eccentricity (:551-559) -- in the host's operations and
 * order, in one call.  in: 22 doubles {left fit a b c, right fit a b c, sum of the window's other valid fits (6), divisor, the seven
 * validity limits, metres per pixel vertical, horizontal}; ploty_v / ploty2_v: plot rows of partial = 1, ploty / ploty2: of the
 * frame's partial; avg6, left_n .. right_yx: the averaged coefficients and their points as lt_poly_points leaves them; out: 5
 * doubles {valid, not-reproduced flag, left radius, right radius, eccentricity}.  With the flag set the caller computes the frame the
 * long way (a radius within 1e-8 of an integer, where upstream's refit decides int(); no plot point inside the image; ...). */
int  lt_frame_tail(int warp_w, int warp_h, const double* in, const double* ploty_v, const double* ploty2_v, int n_rows_v, const double* ploty,
                   const double* ploty2, int n_rows, double* avg6, int32_t* left_n, int32_t* right_n, int32_t* left_yx, int32_t* right_yx,
                   double* out);
/* annotated frames, RGB interleaved, n * img_h * img_w * 3 bytes */
int  lt_download_overlay(lt_ctx* ctx, int first_slot, int n, uint8_t* out);
/* The same copy enqueued behind the slots' overlay work without waiting: `out` (page-locked memory from lt_host_alloc, or
 * the copy is not asynchronous) holds the frames after the next lt_sync / lt_download_*.  lt_overlay_run and lt_overlay_text
 * themselves only enqueue (their staging is per slot), so a window can be rendered and downloaded in pieces while later
 * frames are still searched; a call over slots whose previous overlay is still in flight waits for that one. */
int  lt_download_overlay_async(lt_ctx* ctx, int first_slot, int n, uint8_t* out);
/* The same for two runs of rows of every frame (rows4 = {a0, a1, b0, b1}; NULL: whole frames), at their places in `out`: the
 * other rows of an annotated frame equal the camera frame (lt_overlay_rows) and need not cross the bus -- the caller copies them
 * from the frames it holds (lt_host_copy2d_async). */
int  lt_download_overlay_rows_async(lt_ctx* ctx, int first_slot, int n, uint8_t* out, const int32_t* rows4);
/* Wait until every copy enqueued by lt_download_overlay_async has landed -- and for nothing else: uploads and masks of
 * later frames keep running (lt_sync would drain them too). */
int  lt_download_overlay_wait(lt_ctx* ctx);
/* ---- device sinks: annotated frames into surfaces the caller owns ------------------------------------------------------------
 * The way out that mirrors lt_attach_device_frames: the whole annotated frames of slots -- RGB, dense, in the context's own
 * memory -- are written by a kernel into lt_device_surface destinations in device memory: RGB rows at the caller's pitch, or
 * YUV 4:2:0 as an encoder takes it, NV12 or I420, planes anywhere, any pitch, any byte alignment (16-byte aligned bases and
 * pitches and a width that is a multiple of 16 take the wide kernels).  `layout` is an lt_input_layout -- RGB, NV12, I420, or BGR /
 * RGBA / BGRA (the RGB copy with permuted channels, alpha 255): packed
 * 4:2:2 is an input format only, LT_ERR_INVALID here -- and has nothing to do with
 * the context's input format: an RGB camera may feed an NV12 encoder.  RGB -> YUV is OpenCV's integer arithmetic
 * (cv2.cvtColor(img, COLOR_RGB2YUV_I420), 20-bit fixed point, no chroma averaging):
 *     Y = clamp((CRY r + CGY g + CBY b + 2^19 + (16  << 20)) >> 20)     every pixel
 *     U = clamp((CRU r + CGU g + CBU b + 2^19 + (128 << 20)) >> 20)     of the pixel at (even row, even column) of each 2 x 2 block
 *     V = clamp((CBU r + CGV g + CBV b + 2^19 + (128 << 20)) >> 20)     of the same pixel; its R coefficient IS CBU
 * with coeffs = {CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV} (LT_RGB2YUV_BT601: OpenCV's own; LT_RGB2YUV_BT709; any other matrix
 * whose magnitudes stay below 2^23 and whose rows keep sum |c| * 255 + 2^19 + (128 << 20) inside 32 bits).  coeffs is not read
 * for LT_INPUT_RGB.
 * Every destination plane is checked on the host BEFORE anything is launched, by the rules of lt_attach_device_frames: device
 * memory of that device, known to this runtime, its whole extent -- pitch * (rows - 1) + row bytes -- inside one allocation,
 * pitches at least a row wide and below 2^23; width and height even for 4:2:0; no two planes of a call sharing a byte; and for a
 * context no destination sharing a byte with a camera surface attached to any of its slots (a sink is never the input: drawing in
 * place is lt_overlay_run_inplace's; a slot stays attached until an upload of camera rows or an in-place draw detaches it).  Anything else is LT_ERR_INVALID with a
 * message; a slot that holds only row runs of its annotated frame is LT_ERR_STATE (as for lt_download_overlay); nothing is launched
 * and the context is as it was.  Only bytes inside a row of a plane are ever written: what lies between rows and around planes
 * stays the caller's.
 *   lt_rgb_to_surfaces       n dense RGB frames of h x w (at most 16384 each), frame_stride bytes apart, in a block of
 *                            lt_device_alloc -> dst[0 .. n); synchronous.  For callers without a context, tools, tests.
 *   lt_overlay_store_device  the whole annotated frames of slots [first_slot, first_slot + n) -> dst[0 .. n), enqueued on the
 *                            presentation stream behind the lt_overlay_run / lt_overlay_text that wrote them; returns without
 *                            waiting.  dst[] itself is read before the call returns; the memory it names must stay valid until
 *                            lt_overlay_store_wait, or an lt_sync, has returned -- its content is final then.  A later
 *                            lt_overlay_run over the same slots is ordered behind the store by the stream.
 *   lt_overlay_store_wait    the host waits until every store enqueued so far has landed -- and for nothing else. */
#define LT_RGB2YUV_BT601 {269484, 528482, 102760, -155188, -305135, 460324, -385875, -74448}   /* video range; OpenCV's constants */
#define LT_RGB2YUV_BT709 {191455, 644067, 65019, -105533, -355018, 460551, -418321, -42230}    /* video range; round(c * 2^20) */
int  lt_rgb_to_surfaces(int device, const void* rgb, size_t frame_stride, int h, int w, int n, const lt_device_surface* dst, int layout,
                        const int32_t coeffs[8]);
int  lt_overlay_store_device(lt_ctx* ctx, int first_slot, int n, const lt_device_surface* dst, int layout, const int32_t coeffs[8]);
int  lt_overlay_store_wait(lt_ctx* ctx);
/* ---- annotated frames IN the caller's camera surfaces ------------------------------------------------------------------------
 * The third destination: the surfaces attached to the slots (lt_attach_device_frames) themselves.  An annotated frame differs from
 * its camera frame only where the lane polygon lands -- rows lt_overlay_rows, the green byte -- and under the text lines; the
 * kernels visit those rows only, read the surface where it lies and store only what changed.  There is no destination argument: in
 * place means the input.  RGB, NV12 and I420 contexts, by lt_attach_device_frames' rules (any pitch, any alignment, planes anywhere;
 * 4-byte aligned RGB / 8-byte aligned 4:2:0 geometry takes the wide kernels).
 *   RGB surface    every pixel becomes what lt_overlay_run + lt_overlay_text would have drawn; only bytes of pixels that change
 *                  are written; nothing between rows or around the plane.
 *   4:2:0 surface  with C = the camera frame as RGB (the context's input matrix) and A = C with lane and text drawn: Y of pixel p
 *                  becomes luma(A(p)) where A(p) != C(p); the (U, V) of a 2 x 2 block become chroma(A(top-left pixel)) where that
 *                  pixel changed -- the bytes lt_overlay_store_device would write there (rgb2yuv[8] as its coeffs; not read by an RGB
 *                  context).  Every other byte keeps what the decoder wrote: YUV -> RGB -> YUV is not the identity, and it is
 *                  applied to nothing that was not drawn on.  A block under both the lane and the text is converted once, drawn on
 *                  twice, converted back once.
 * text: NULL or n_lines <= 0 for none; else n_lines * line_len bytes per slot (NUL-padded) as for lt_overlay_text, the first line's
 * top left at (x0, y0), `step` rows between lines -- at least the glyph height (LT_ERR_INVALID); characters behind a line's first
 * NUL are not drawn.  Needs lt_overlay_set_font.
 *   lt_overlay_run_inplace         the lanes as plot points (lt_overlay_run's arguments)
 *   lt_overlay_run_inplace_coeffs  the lanes as averaged coefficients (lt_overlay_run_strip_coeffs' arguments; LT_ERR_STATE where
 *                                  that form does not exist)
 * Refusals, all before anything is staged or launched (the context and the surfaces are as they were): LT_ERR_STATE for a slot
 * that is not attached or whose calibration set's overlay is not configured; LT_ERR_INVALID for bad point lists, missing or
 * oversized rgb2yuv (4:2:0), a NULL text or overlapping lines.
 * Enqueued on the presentation stream, behind the front end of exactly these slots: the undistortion lt_mask_run enqueued for a
 * frame has read the surface before a byte of it changes.  Returns without waiting; lt_overlay_store_wait and lt_sync cover these
 * draws as they cover lt_overlay_store_device's stores -- the surfaces are final, and the caller's again, when one has returned.
 * Afterwards the slots are DETACHED and marked: their surfaces hold no camera frame any more.  lt_mask_rerun still works (the
 * planes of the front end came from the original pixels); lt_mask_run and lt_device_frames_rest over such a slot are LT_ERR_STATE
 * until an attach or an upload brings a new frame; a later lt_overlay_store_device may write into the surface. */
typedef struct lt_inplace_text {
    const char* lines;
    int32_t n_lines, line_len, x0, y0, step;
} lt_inplace_text;
int  lt_overlay_run_inplace(lt_ctx* ctx, int first_slot, int n, const int32_t* left_n, const int32_t* right_n, const int32_t* left_yx,
                            const int32_t* right_yx, double alpha, const lt_inplace_text* text, const int32_t rgb2yuv[8]);
int  lt_overlay_run_inplace_coeffs(lt_ctx* ctx, int first_slot, int n, const double* coeffs, const uint8_t* draw, const double* ploty,
                                   const double* ploty2, int n_rows, double alpha, const lt_inplace_text* text, const int32_t rgb2yuv[8]);
/* ---- annotated frames drawn on their way INTO device sinks -----------------------------------------------------------------------
 * lt_overlay_run + lt_overlay_text + lt_overlay_store_device as one pass: every pixel of the camera frames of slots [first_slot,
 * first_slot + n) is read once, drawn on -- the lane with the inverse-warp table of the slot's OWN calibration set, then the text --
 * and written straight into dst[0 .. n) in `layout` (RGB at its pitch; NV12 / I420 with coeffs[8], chroma from the pixel at the even
 * row and even column): byte for byte what the three calls leave in the sinks.  No annotated frame is kept in the context
 * (lt_download_overlay and lt_overlay_store_device do not see these frames), and one kernel launch serves up to 32 slots whatever
 * their sets.  `text` as for lt_overlay_run_inplace (NULL: none).
 * Preconditions, refusals and ordering are those of lt_overlay_run followed by lt_overlay_store_device: whole camera frames in the
 * slots and every slot's set configured (LT_ERR_STATE), the sinks' rules above -- layout, even sizes and coefficients for 4:2:0,
 * pitches, disjoint planes, no byte shared with an attached camera surface (LT_ERR_INVALID) -- all checked before anything is
 * staged or launched: a refused call leaves the context and the surfaces as they were.  Enqueued on the presentation stream behind
 * the slots' writers and pending lt_upload_frame_rest / lt_device_frames_rest copies; returns without waiting; the surfaces are
 * final after lt_overlay_store_wait or lt_sync. */
int  lt_overlay_run_to_surfaces(lt_ctx* ctx, int first_slot, int n, const int32_t* left_n, const int32_t* right_n, const int32_t* left_yx,
                                const int32_t* right_yx, double alpha, const lt_inplace_text* text, const lt_device_surface* dst, int layout,
                                const int32_t coeffs[8]);
/* How lt_download_overlay_async moves the frames: 0 = the copy engine, 1 = a kernel storing into the (page-locked, 16-byte
 * aligned) destination, -1 (default) = chosen by measurement: every copy is timed, the engine is used while its copies
 * reach ~42 GB/s, otherwise whichever of the two measures faster (the engine's rate depends on how the process's memory
 * happens to be laid out: 28-56 GB/s; the kernel reaches 38-40 GB/s regardless).  lt_download_stats reports the running
 * rates (GB/s), the number of timed copies per method and the method the next copy would use; any pointer may be NULL. */
int  lt_set_download_method(lt_ctx* ctx, int method);
int  lt_download_stats(lt_ctx* ctx, double* engine_gbs, int* engine_copies, double* kernel_gbs, int* kernel_copies, int* method);
/* ---- annotated frames of a window as strips (round 5) ----------------------------------------------------------------------
 * Outside the rows the lane can reach (lt_overlay_rows) an annotated frame is the camera frame plus the text lines -- both of
 * which the host has.  So of an annotated frame only that run of rows is drawn on the device, packed ("strip", rows * img_w * 3
 * bytes per slot), and it comes back as ONE contiguous copy per block of 32 slots into page-locked staging blocks the library
 * pools (copy engine, full rate), from where the library's copy threads put the rows into the caller's frames -- ordinary
 * memory: no window-sized page-locked output array (0.13 s of page-locking per 0.7 GB, the first window's largest cost).  The
 * other rows and the text the caller adds with lt_host_copy2d_async_group / lt_host_text_async_group in the same group;
 * lt_host_copy_wait_group(group) returns when the frames are complete.  Needs img_w % 4 == 0.
 *   lt_overlay_run_strip     lt_overlay_run for rows [lt_overlay_rows) only, into the context's strip buffer
 *   lt_strip_download_async  the strips of slots [first, first + n) -> rows [row0, row1) of out + i * out_frame_stride (i < n)
 *   lt_overlay_run_strip_coeffs  lt_overlay_run_strip from the lanes' AVERAGED coefficients (n x 6 doubles: left a, b, c, right
 *                            a, b, c; :1182-1189) instead of their plot points: get_poly_points (:511-528; ploty / ploty2 as for
 *                            lt_present_lane_from_fit_async) and the polygons' row intervals are formed on the device, one
 *                            workgroup per frame.  draw: n bytes, 0 = no lane in that frame (nullptr: all drawn).  LT_ERR_STATE
 *                            where that form does not exist (an odd bird's-eye height): use the points form */
int  lt_overlay_run_strip(lt_ctx* ctx, int first_slot, int n, const int32_t* left_n, const int32_t* right_n, const int32_t* left_yx,
                          const int32_t* right_yx, double alpha);
int  lt_overlay_run_strip_coeffs(lt_ctx* ctx, int first_slot, int n, const double* coeffs, const uint8_t* draw, const double* ploty,
                                 const double* ploty2, int n_rows, double alpha);
int  lt_strip_download_async(lt_ctx* ctx, int first_slot, int n, uint8_t* out, size_t out_frame_stride, int group);
/* The text lines of draw_lane() / print_failure() (lane_tracker.py:652-661, 664-673; glyph atlas as for lt_overlay_set_font) drawn on
 * the HOST, with lt_overlay_text's arithmetic bit for bit (white over the frame: v + ((255 - v) * alpha + 127) / 255): `lines` holds
 * n_lines * line_len bytes per frame (NUL-padded), frame after frame.  No GPU, no context.
 *   lt_text_blend_host        n frames in place, on the calling thread (LaneTracker.process(): ~10 us per frame)
 *   lt_host_text_async_group  on the library's copy threads, in `group`: per frame, first copy two runs of rows {a0, a1, b0, b1}
 *                             (rows4; NULL or empty runs: nothing) of the source frame into the destination frame -- every row
 *                             the device does not deliver: above and below the lane's run -- then draw the lines over them.
 *                             `lines` is copied; the frames and the atlas must stay valid until the group's wait.
 *   lt_host_text_now_group    ONE frame, now: waits for `group` (whose copies bring the rows under the text), then draws the lines --
 *                             the first on the calling thread, the others on copy threads that are polling at that moment (or here);
 *                             returns with the text drawn.  LaneTracker.process(): no job, no second wait. */
int  lt_text_blend_host(uint8_t* frames, size_t frame_stride, int n, int img_h, int img_w, const uint8_t* atlas, const uint8_t* advance,
                        int first_char, int n_glyphs, int glyph_w, int glyph_h, const char* lines, int n_lines, int line_len, int x0,
                        int y0, int step);
int  lt_host_text_async_group(int group, uint8_t* dst, size_t dst_stride, const uint8_t* src, size_t src_stride, int n, const int32_t* rows4,
                              int img_h, int img_w, const uint8_t* atlas, const uint8_t* advance, int first_char, int n_glyphs,
                              int glyph_w, int glyph_h, const char* lines, int n_lines, int line_len, int x0, int y0, int step);
int  lt_host_text_now_group(int group, uint8_t* frame, int img_h, int img_w, const uint8_t* atlas, const uint8_t* advance, int first_char,
                            int n_glyphs, int glyph_w, int glyph_h, const char* lines, int n_lines, int line_len, int x0, int y0, int step);
/* Page-locked host memory for buffers passed to the upload / download entry points (copies from or to pageable
 * memory run at a fraction of the PCIe rate).  Needs a GPU; lt_host_free(NULL) is a no-op.  The reference has no
 * counterpart: its frames are NumPy arrays on the host (lane_tracker.py:876, :662). */
int  lt_host_alloc(size_t bytes, void** out);
/* Plain host-to-host copies on a second host thread of the library (one per process), for a caller that has launches to issue
 * meanwhile: LaneTracker.process() fills the rows of its output that no overlay can touch from the camera frame this way.
 * lt_host_copy_async returns at once; both buffers must stay valid until lt_host_copy_wait() has returned, which is when every
 * copy requested so far (by any thread) is complete. */
int  lt_host_copy_async(void* dst, const void* src, size_t bytes);
/* height pieces of width bytes, dst_pitch / src_pitch bytes apart (a run of rows of every frame of a window), shared among
 * the library's copy threads (LT_COPY_THREADS, default 4) */
int  lt_host_copy2d_async(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t height);
int  lt_host_copy_wait(void);
/* The same copies with completion per GROUP: a copy belongs to the group it is submitted to, and lt_host_copy_wait_group(g)
 * returns when the copies of g are complete -- whatever other trackers, threads or windows have queued meanwhile (with one
 * counter per process, two trackers on two threads waited for each other's copies and a short wait could be starved by
 * another tracker's 360 MB window).  Group 0 is the default group lt_host_copy_async / lt_host_copy2d_async submit to;
 * lt_host_copy_wait() waits for every group.  lt_host_copy_group_create hands out a fresh id (> 0, never reused);
 * lt_host_copy_group_destroy waits for the group and forgets it.  An unknown group is LT_ERR_INVALID.  No GPU needed.
 * LaneTracker keeps one group per tracker for process() and one per window of a stream. */
int  lt_host_copy_group_create(int* group);
int  lt_host_copy_group_destroy(int group);
int  lt_host_copy_async_group(int group, void* dst, const void* src, size_t bytes);
int  lt_host_copy2d_async_group(int group, void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t height);
int  lt_host_copy_wait_group(int group);
/* Write one byte into every 4 KB page of [p, p + bytes) on the copy threads: first touch of fresh memory ahead of its use (the
 * output frames of a stream's first windows; ~10 GB/s whatever the thread count).  The contents are undefined afterwards. */
int  lt_host_touch_async_group(int group, void* p, size_t bytes);
/* Finish the queued host copies and join the copy threads now (they are also joined when the library is unloaded, and start
 * again with the next request).  For hosts that must not have library threads alive at a point of their choosing -- before a
 * fork(), at interpreter shutdown.  (The child of a fork() gets fresh workers by itself: pthread_atfork.) */
int  lt_shutdown(void);
/* Since the process started: seconds the copy threads spent on pieces (summed over the threads), bytes of plain copies, pieces
 * run, and the number of threads requests are shared among (LT_COPY_THREADS; default half of the CPUs the process may use,
 * 2 .. 8).  Any pointer may be NULL.  bench.py reports the copy threads' share of an annotated stream from these. */
int  lt_host_copy_stats(double* busy_seconds, double* copied_bytes, long long* pieces, int* threads);
/* What the library holds on the host right now: page-locked staging blocks it has allocated (bytes; strips of annotated frames
 * travel through them), pieces waiting in the copy threads' queue, and pieces submitted or reserved but not finished.  A
 * long-lived process sees the first flat and the other two back at 0 between windows (tests/test_gpu_soak.py).  Any pointer
 * may be NULL. */
int  lt_host_memory_stats(size_t* staging_bytes, size_t* queued_pieces, size_t* pending_pieces);
int  lt_host_free(void* p);
/* Device memory a context gives up (lt_destroy, lt_reserve growing) is kept in a per-process cache, by device and exact
 * size, and reused by later allocations.  Why: memory handed back to the driver is wiped in the background on an SDMA engine,
 * and for that time the process's device-to-host copies run at half speed (csrc/lt_memory.cpp, DevCache).  The cache keeps at
 * most the high-water mark of what the process's live contexts have held at once, and at most 16 GB (LT_DEVICE_CACHE_GB=<n>:
 * another limit; 0: no cache); beyond that the blocks that have waited longest go back to the driver.  lt_device_cache_trim
 * returns everything beyond keep_bytes NOW -- for a process that shares the GPU (several ranks on one device, another
 * allocator in the same process): call it with 0 after closing trackers whose memory somebody else should have.  A failed
 * hipMalloc inside the library trims by itself and tries once more.  lt_device_cache_stats: bytes the cache holds, bytes handed
 * out to live contexts, the current limit, the number of cached blocks (any pointer may be NULL).  No context needed. */
int  lt_device_cache_trim(size_t keep_bytes);
int  lt_device_cache_stats(size_t* kept_bytes, size_t* live_bytes, size_t* limit_bytes, int* kept_blocks);
/* Since the process started: allocations served from the cache, allocations that went to hipMalloc, and what the cache gave
 * back to the driver (evictions over its limit, lt_device_cache_trim) -- a long-lived process that keeps evicting pays the
 * driver's wipe with half-rate device-to-host copies each time (tests/test_gpu_soak.py holds these flat).  Any pointer may be NULL. */
int  lt_device_cache_counters(unsigned long long* hits, unsigned long long* misses, unsigned long long* evicted_blocks,
                              unsigned long long* evicted_bytes);
/* the bird's-eye RGB image of the slots' frames (lane_tracker.py:834, :1035): n * warp_h * warp_w * 3;
 * needs lt_mask_run on those slots first (it reuses their undistorted rows) */
int  lt_download_bev(lt_ctx* ctx, int first_slot, int n, uint8_t* out);
/* The search visualisations of listed frames (visualize_sliding_window_search / visualize_band_search, lane_tracker.py:687-771),
 * painted on the device from what the slots hold -- the opened mask, the lane pixels in whatever form the search left them, the
 * window centroids -- and sent to out_host: n pictures of warp_h * warp_w * 3 bytes, in item order.  The point lists are int32
 * (y, x) pairs, the items' points back to back: the plot points of the new left / right fit (yellow), and for kind 2 those of the
 * curves the band was searched around (lt_poly_points produces all four).  A kind-0 picture is the mask in all three channels.
 * Enqueued behind everything launched so far over each listed slot; work launched over those slots later is ordered behind the
 * reads.  `items` and the lists are read before the call returns.  The copies run on the download stream: out_host holds the
 * pictures after lt_search_viz_wait, lt_sync or an lt_download_* call (page-locked memory preferred, pageable taken).  The
 * pictures pass through a staging ring of 32 frames, allocated by the first call and freed by lt_reserve / lt_destroy: nothing
 * grows with the capacity, and a longer list goes through the ring in pieces.  LT_ERR_INVALID: n < 0, a NULL list that is
 * needed, a slot outside the capacity, an unknown kind, a negative count, window_height <= 0 (kind 1); LT_ERR_STATE: a slot
 * without a mask, kinds 1 / 2 before any search has run.  Nothing is launched after a refusal. */
int  lt_search_viz_run(lt_ctx* ctx, int n, const lt_viz_item* items, const int32_t* fit_left_yx, const int32_t* fit_right_yx,
                       const int32_t* band_left_yx, const int32_t* band_right_yx, uint8_t* out_host);
/* The same pictures as the lower part of triple_split_view (lane_tracker.py:773-793): per item one strip of scaled_h * img_w * 3
 * bytes -- the bird's-eye RGB image (as lt_download_bev) scaled to (scaled_w, scaled_h) at column 0, the visualisation scaled
 * likewise at column second_x, both cropped at the right edge, bytes no pane covers 0 (lt_split_panes_size gives the three
 * numbers; cv2.resize INTER_LINEAR arithmetic).  Same contract as lt_search_viz_run; the slots need lt_mask_run first. */
int  lt_split_panes_run(lt_ctx* ctx, int n, const lt_viz_item* items, const int32_t* fit_left_yx, const int32_t* fit_right_yx,
                        const int32_t* band_left_yx, const int32_t* band_right_yx, uint8_t* out_host);
int  lt_split_panes_size(lt_ctx* ctx, int* scaled_w, int* scaled_h, int* second_x);   /* no GPU work; any pointer may be NULL */
int  lt_search_viz_wait(lt_ctx* ctx);  /* waits for the copies of the two calls above, and for nothing else */

/* ---- host-only views of the calibration tables (no GPU needed) --------------------------------------- */
/* What lt_create derives from the calibration, exposed so that it can be checked against independent
 * generators (tests/test_tables_independent.py): the cv::remap fixed-point maps -- xy: (sx, sy) int16 pairs,
 * frac: fy*32 + fx -- of cv2.warpPerspective (:834; warp_h*warp_w entries) and of cv2.undistort (:832; rows
 * [row0,row1) x img_w entries), the camera rows the warp reads, the RGB2LAB tables (:208) and the half-widths
 * of getStructuringElement(MORPH_ELLIPSE, (k,k)) (:203-205). */
int  lt_calib_source_rows(const lt_calib* calib, int* row0, int* row1);
/* lt_split_panes_size for a calibration (only the four sizes are read): triple_split_view's arithmetic (:781-787) */
int  lt_calib_split_panes_size(const lt_calib* calib, int* scaled_w, int* scaled_h, int* second_x);
int  lt_calib_warp_table(const lt_calib* calib, int16_t* xy, uint16_t* frac);
int  lt_calib_undistort_table(const lt_calib* calib, int row0, int row1, int16_t* xy, uint16_t* frac);
int  lt_calib_lab_tables(uint16_t* gamma256, uint16_t* cbrt3072, int32_t* coeffs9);
int  lt_calib_ellipse(int k, int32_t* halfwidths /* k */, int* taps);

/* ---- multi-GPU: the gather of the lane records ------------------------------------------------------ */
/* Independent frames shard over the GPUs of one node by contiguous index blocks with no data-path exchange
 * (SURVEY 8(e)); the only collective is this all-gather of the 64-byte lane records, run on RCCL (librccl.so is
 * opened by lt_gather_init, so single-GPU users never load it).  The reference has no counterpart: it is one
 * Python process (process_video.py:41-44).  One lt_gather per rank = per process = per GPU, bound to the
 * context whose records it moves.
 *
 * lt_gather_init: rank 0 creates the RCCL id and publishes it at id_path (temporary name + rename); the other
 * ranks wait up to timeout_s (<= 0: 120 s) for that file.  Every rank of the job must call it (collective). */
typedef struct lt_gather lt_gather;
int  lt_gather_init(lt_ctx* ctx, int rank, int world, const char* id_path, int timeout_s, lt_gather** out);
int  lt_gather_world(lt_gather* g, int* rank, int* world);
/* staging capacity: records per rank (e.g. steps * frames per step); identical on every rank */
int  lt_gather_reserve(lt_gather* g, int records_per_rank);
/* Copy the records of context slots [first_slot, first_slot + n) to position `at` of the send buffer,
 * enqueued behind the slots' searches on the context's streams -- no host wait. */
int  lt_gather_stage(lt_gather* g, int first_slot, int n, int at);
/* ONE ncclAllGather of the first n_records staged records of every rank (the same n_records everywhere; pad
 * uneven shards), after the context's streams have drained the staged copies.  out_host receives
 * world * n_records records, rank-major.  Collective; synchronises. */
int  lt_gather_records(lt_gather* g, int n_records, lt_lane_record* out_host);
/* All-gather of `bytes` host bytes per rank (timings, checksums): out holds world * bytes.  Collective. */
int  lt_gather_host(lt_gather* g, const void* in, size_t bytes, void* out);
/* lt_sync of the bound context, then a collective round trip: no rank returns before every rank has arrived */
int  lt_gather_barrier(lt_gather* g);
void lt_gather_destroy(lt_gather* g);

/* ---- measurement ------------------------------------------------------------------------------ */
/* hipEvent pair on the context's stream */
int  lt_timer_start(lt_ctx* ctx);
int  lt_timer_stop(lt_ctx* ctx, float* ms);
/* when enabled, every *_run records a hipEvent after each kernel; lt_stage_ms returns the
 * accumulated milliseconds and launch counts per stage since the last lt_stage_reset */
int  lt_set_stage_timing(lt_ctx* ctx, int enabled);
int  lt_stage_reset(lt_ctx* ctx);
int  lt_stage_ms(lt_ctx* ctx, float* ms, int32_t* launches, int n);
const char* lt_stage_name(int stage);
/* Which kernels evaluated the bilateral thresholds in the context's last 'bilateral' lt_mask_run / lt_filter_run:
 * 1 = the long-walk kernels (window sizes 15 / 20 / 35, width a multiple of 4; with the greenery mask -- mask_noise,
 * lane_tracker.py:221-231 -- when its window is 65), 0 = the tile kernel, -1 = none yet; LT_NO_CONTEXT for a null
 * context (distinct from every status and from "none yet").  Both give identical masks; tests use this to know which
 * one they have exercised. */
#define LT_NO_CONTEXT (-2147483647 - 1)
int  lt_last_threshold_path(lt_ctx* ctx);
/* Which form of them: 0 = the tile kernel, 1 = the running-sum walks, 2 = the matrix-core form (the window sums as i8 band
 * products; where lt_last_threshold_path says 1 and the walks' conditions hold), -1 = none yet; LT_NO_CONTEXT for a null
 * context.  Forms 1 and 2 write identical partial planes; the greenery mask keeps its running-sum walk under either. */
int  lt_last_threshold_form(lt_ctx* ctx);
/* Which form of the 5x5 open the last slice of the context's last lt_mask_run / lt_filter_run launched: 0 = the separate kernels
 * (the merge, the erode and the dilate a launch each: 5 to 15 frames, and every plane that reaches the open merged already),
 * 1 = the wave walk (merge + open in one pass, 16 frames or more), 2 = the small form (merge + open in one launch of small
 * workgroups, up to 4 frames), -1 = none yet; LT_NO_CONTEXT for a null context.  All three give identical masks and merged
 * planes; tests use this to know which one they have exercised.  (lt_filter_lane_points does not report here.) */
int  lt_last_open_form(lt_ctx* ctx);
/* Which form of the batch top-hat walks the context's last lt_mask_run / lt_filter_run piece launched: bit 0 = the 29x29 pair
 * of launches, bit 1 = the 55x55 pair took the split-band form (every band walks its own rows only and boundary rows are
 * merged from the two neighbours' partial results); 0 = the bands walked their halos, or another top-hat route ran (one or two
 * frames, brute force); -1 = none yet.  Both forms give identical planes. */
int  lt_last_tophat_path(lt_ctx* ctx);
/* The host's rule behind it, callable without a device: 1 if an h x w plane cut into `nbands` bands takes the split-band form
 * of the k x k walk (k = 29 or 55): rows 4-byte aligned, at most four bands, every band -- the last, shorter one included --
 * at least one boundary zone (28 / 56 rows) long. */
int  lt_tophat_split_form(int h, int w, int k, int nbands);
/* The same for the last 'neighborhood' call (cv2.adaptiveThreshold, lane_tracker.py:217-218): 1 = running box sums
 * (odd windows up to 63, width a multiple of 4, no greenery mask), 0 = the per-pixel window kernel, -1 = none yet. */
int  lt_last_adaptive_path(lt_ctx* ctx);
/* What the kernels of the context's last lt_sws_fit_run, lt_band_fit_run, lt_band_fit_chain_run or lt_search_fit_list read: 1 = the
 * bit planes of every slot searched, 0 = the u8 mask of at least one (a slot filled by lt_upload_masks, a geometry the bit-plane
 * kernels do not take -- a window or band wider than 64 columns, ... -- or a
 * list whose slots are not all bit planes), -1 = none yet; a refused call or one over no slots does not change it; LT_NO_CONTEXT
 * for a null context.  Both give identical results (above); tests use this to know which kernels they have exercised. */
int  lt_last_search_source(lt_ctx* ctx);
/* The lane-drawing kernel launches the most recent lt_overlay_run, lt_overlay_run_rows, lt_overlay_run_inplace,
 * lt_overlay_run_inplace_coeffs or lt_overlay_run_to_surfaces of the context enqueued (text and store launches are not counted):
 * 1 for a range of up to 64 slots (32 for lt_overlay_run_to_surfaces) whatever the slots' calibration sets -- a range that mixes
 * sets is drawn by table-per-slot kernels, not run by run.  -1 = none yet; a refused call does not change it; LT_NO_CONTEXT for a
 * null context. */
int  lt_last_overlay_launches(lt_ctx* ctx);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
