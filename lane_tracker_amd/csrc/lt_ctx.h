// The context behind the C ABI (struct lt_ctx) and the helpers its translation units share:
//   lt_api.cpp     -- create / destroy / reserve, input format and size, downloads, the searches, measurement
//   lt_raw.cpp     -- what raw Bayer frames are conditioned with (raw table, colour stage, shading map: raw_setup.h), raw statistics, the
//                     one-shot converters of a host frame to RGB
//   lt_ingest.cpp  -- host frames into slots: lt_upload_frames, the row and rest uploads, lt_device_frames_rest (direct, staged, resized)
//   lt_mask_chain.cpp -- the mask chain (top-hats, thresholds, merge + 5x5 open) and the arena that owns its device memory
//   lt_memory.cpp  -- device-memory cache, page-locked host memory, the host copy threads
//   lt_present.cpp -- presentation stage: lane overlay, text, annotated frames on their way back
//   lt_chain.cpp   -- the chained band search of a stream (tickets, cancel, collect)
//   lt_search_viz.cpp -- search visualisations and split-view panes of listed frames, lt_resize_linear_u8
//   lt_sink.cpp    -- device sinks: annotated frames (or any RGB frames) into the caller's RGB / NV12 / I420 surfaces; the checks of
//                     a call's destinations (shared with lt_overlay_run_to_surfaces, lt_present.cpp)
// Not installed; the public ABI is include/lane_tracker_amd.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <vector>

#include "lt_internal.h"

namespace lt {

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // fills lt_last_error(), returns code

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return lt::fail(LT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

enum Stage {
    ST_UNDISTORT = 0, ST_WARP_SPLIT, ST_ERODE_R, ST_TOPHAT_R, ST_ERODE_B, ST_TOPHAT_B, ST_THRESHOLD, ST_MERGE,
    ST_OPEN, ST_SWS_FIT, ST_BAND_FIT, ST_SPLIT_BEV
};

enum Plane { P_R = 0, P_B, P_THR, P_THB, P_MERGED, P_MASK, P_T0, P_T1, P_T2, P_T3, P_COUNT };

// The device memory the mask chain (lt_mask_chain.cpp) reads and writes, for `capacity` slots of h x w pixels: a context holds
// one for its slots, lt_filter_lane_points a one-slot one for the length of a call.  Whatever the chain allocates on the way
// lands here, and release() is the only place that frees any of it.
struct MaskArena {
    int capacity = 0;
    size_t plane_bytes = 0;           // h * w
    size_t bits_stride = 0;           // u64 words per slot of a bit plane: 1 bit / pixel, wpr words per row
    uint8_t* d_plane[P_COUNT] = {};   // P_R, P_B, P_THR, P_THB, P_T0 from reserve(); the others on first use (ensure_plane)
    unsigned long long *d_bits_merged = nullptr, *d_bits_eroded = nullptr;
    unsigned long long* d_bits_open = nullptr;    // the opened mask as the chain leaves it (what the searches read)
    unsigned long long* d_bits_tmp = nullptr;     // third and fourth partial plane of the walking threshold kernels
    unsigned long long* d_bits_tmp2 = nullptr;
    // Top-hat planes with a 64-byte-multiple row pitch: what the walking threshold kernels read (every 64-byte piece of
    // a row is one aligned sector; with the image width as pitch the horizontal pass fetched every sector twice).
    // th_padded[slot] says which copy of the slot's top-hat planes is current (lt_download_plane).
    uint8_t* d_th_pad[2] = {nullptr, nullptr};
    size_t th_pad_bytes = 0;
    int th_pitch = 0;
    std::vector<uint8_t> th_padded;
    // mask_noise through the walking kernels (allocated by the first such call, ensure_noise_buffers): the raw Lab-b plane
    // in the padded layout (the 55x55 top-hat launch stores its minuend there) and the two greenery-mask bit planes
    uint8_t* d_b_pad = nullptr;
    unsigned long long *d_bits_n1 = nullptr, *d_bits_n2 = nullptr;
    // the eroded R plane of a one- or two-frame chain: two planes per stream that can run one (ensure_side_scratch)
    static constexpr int SIDE_LANES = 10;         // one per slice stream (up to 8), one for every other stream
    uint8_t* d_side_scratch = nullptr;
    // the boundary zones of the split-band top-hat walks (k_tophat.hip: k_morph_split): per slot and 128-column strip three zones
    // of 56 rows x 64 dwords; the four launches of a slot's chain run one behind the other and share them (ensure_zone_scratch)
    uint32_t* d_zone = nullptr;
    size_t zone_stride = 0;                       // dwords per slot

    MaskArena() = default;
    MaskArena(const MaskArena&) = delete;
    MaskArena& operator=(const MaskArena&) = delete;
    ~MaskArena() { release(); }
    void set_geometry(int h, int w);              // the sizes above; allocates nothing
    // the planes every call needs; batch: also the opened bit plane and what the walking kernels of large calls read and write
    int reserve(int slots, bool batch);
    void release();                               // frees everything; the geometry stays
    bool walk_planes() const { return d_th_pad[0] && d_th_pad[1] && d_bits_tmp && d_bits_tmp2; }
    int ensure_plane(int idx);
    int ensure_noise_buffers();
    int ensure_side_scratch();
    int ensure_zone_scratch();
};

// The staging ring of lt_search_viz_run / lt_split_panes_run (lt_search_viz.cpp): FRAMES pictures (and, for split views, as many
// bird's-eye images and pane strips) in two halves that take turns -- one is painted while the other crosses the bus.  Allocated
// by the first call that needs a part; nothing here grows with the context's capacity.
struct VizRing {
    static constexpr int FRAMES = 32, HALF = FRAMES / 2;
    uint8_t *d_pics = nullptr, *d_bev = nullptr, *d_panes = nullptr;
    int32_t *d_xt = nullptr, *d_yt = nullptr;      // resize taps bird's-eye size -> pane size (four int32 per column / row)
    struct Half {
        uint8_t *h_stage = nullptr, *d_stage = nullptr;   // band intervals and plot points of the half's pictures: page-locked, device
        size_t h_bytes = 0, d_bytes = 0;
        hipEvent_t staged = nullptr;     // behind the kernels that read the staging and paint the half
        hipEvent_t copied = nullptr;     // behind the copy of the half's pictures to the host
        bool staged_set = false, copied_set = false;
    } half[2];
    int next = 0;
    hipEvent_t last = nullptr;           // the `copied` event of the most recent piece (lt_search_viz_wait); null: nothing in flight
};

}  // namespace lt

using lt::P_COUNT;

struct lt_ctx {
    lt_calib calib{};
    int device = 0;
    hipStream_t stream = nullptr;             // = streams[0]
    std::vector<hipStream_t> streams;         // slot s runs on streams[s * nstreams / capacity]
    hipStream_t copy = nullptr;               // lt_upload_frame_rest: the rows the path does not read, off the critical path
    // One frame's rows written by the calling thread straight into the slot through the PCIe aperture (lt_upload_frame_rows_enqueue of
    // a small call; lt_set_direct_upload): -1 = not yet decided for the current frame buffer, 0 = no (no large BAR, the buffer is
    // not mapped into this process, or switched off), 1 = yes.
    int direct_upload = -1;
    bool direct_upload_wanted = true;
    unsigned long long lane_spec_reader_seq = 0;   // readers.lazy_seq when the completion word of lt_present_lane_from_fit_async was launched
    unsigned long long direct_uploads = 0;    // calls that took the aperture (lt_set_direct_upload(ctx, -1) reports the state, tests read this through it)
    int nstreams = 1;
    hipDeviceProp_t prop{};
    lt::FrontEndGeom fe{};
    int cam_r0 = 0, cam_r1 = 0;               // camera rows the undistortion reads (its taps for rows [fe.r0, fe.r0 + nrows))
    lt::EllipseSE se5{}, se29{}, se55{};
    // device tables
    int16_t *d_uxy = nullptr, *d_wxy = nullptr;
    uint16_t *d_ufrac = nullptr, *d_wfrac = nullptr, *d_gamma = nullptr, *d_cbrt = nullptr;
    int32_t* d_coef = nullptr;
    // Calibration sets (lt_add_calibration).  Set 0 is the context's own: `calib` and the tables above.  `cal[id]` holds what set
    // id brings: its calibration, its remap tables and its overlay table; cal[0] mirrors the pointers above (refresh_cal0).  The
    // geometry is ONE for all sets: fe.r0 / fe.nrows, cam_r0 / cam_r1 and ov_r0 / ov_r1 are the unions over the sets, and every
    // set's undistortion table is built for the union rows.  d_cal: the sets' tables as the table-per-slot kernels read them
    // (allocated with the second set); slot_cal: the set of every slot.
    struct CalSet {
        lt_calib calib{};
        int16_t *d_uxy = nullptr, *d_wxy = nullptr, *d_oxy = nullptr;
        uint16_t *d_ufrac = nullptr, *d_wfrac = nullptr, *d_ofrac = nullptr;
        int r0 = 0, r1 = 0;                   // the rows of the undistorted image its warp reads
        int need0 = 0, need1 = 0;             // the camera rows its undistortion reads for them
        int ov_r0 = 0, ov_r1 = 0;             // the camera rows its lane overlay can change
        bool have_overlay = false;
    };
    std::vector<CalSet> cal;
    lt::CalTables* d_cal = nullptr;
    std::vector<uint8_t> slot_cal;
    // the sets' inverse-warp tables as the table-per-slot presentation kernels read them: entry id written when lt_overlay_configure_set
    // builds set id's tables (allocated by the first such call)
    lt::OvTables* d_ov = nullptr;
    int last_overlay_launches = -1;               // lt_last_overlay_launches
    bool lab_clamp_dead = false;   // no pixel reaches the clamp of the cube-root table index with these tables (front_arith.h)
    // slots
    int capacity = 0;
    size_t frame_bytes = 0, und_bytes = 0, bev_bytes = 0;
    uint8_t *d_frames = nullptr, *d_bev = nullptr;
    // Input that is not RGB (lt_set_input_format): the caller's layout, the five conversion coefficients (YUV), and per slot a staging frame
    // of yuv_bytes = h * w * 3 / 2 (4:2:0), h * w * 2 (packed 4:2:2), h * w * 3 (BGR), h * w * 4 (RGBA / BGRA), h * w (raw Bayer) or 2 * h * w (10- / 12-bit raw Bayer) bytes in that layout, yuv_stride (a multiple of 16) apart, 16 bytes of padding behind the last
    // one (k_undistort_rows reads aligned 8-byte windows).  The undistortion reads the staging frame; the RGB camera frame
    // of a slot is written by k_rows_to_rgb behind the uploads that would have brought RGB rows for whoever shows the frame.
    int in_layout = 0;                        // LT_INPUT_RGB
    int32_t yuv_coef[5] = {0, 0, 0, 0, 0};
    bool input_locked = false;                // an upload has happened: the format stays
    uint8_t* d_yuv = nullptr;
    size_t yuv_bytes = 0, yuv_stride = 0;
    // What a raw Bayer context's frames are conditioned with (lt_raw.cpp: lt_set_raw_lut / _wide, lt_set_raw_color, lt_set_raw_shading, and
    // lt_set_input_format, which starts it afresh): the host value and what it is on the device -- one buffer of what the raw kernels stage in
    // LDS, and the gain plane of the shading map (raw_setup.h).  Every setter edits a copy of `raw`, raw_adopt writes that to the device and
    // makes it the context's; raw_stages_of is what the launches read.  raw.layout is in_layout while that is a raw layout.
    lt::RawSetup raw;
    lt::RawDevice raw_dev;
    // Raw sets (lt_add_raw_set), held as calibration sets are: set 0 is `raw` / `raw_dev` above, sets 1 .. are raw_more[id - 1]; slot_raw: the
    // set of every slot.  A launch whose slots have ONE set runs today's kernels with that set's RawStages (raw_stages_of); one that mixes sets
    // runs the set-per-slot forms with the stages of the union of the sets (raw_union) and reads d_raw_sets, one RawSetEntry per set, written by
    // raw_sets_refresh behind every change: a set whose own staged bytes are not the union's form has them again in that form (union_table),
    // and the sets without a map share d_unit_gain, one plane of unit gains.
    struct RawSet {
        lt::RawSetup s;
        lt::RawDevice d;
    };
    std::vector<RawSet> raw_more;
    struct UnionTable { uint32_t* p = nullptr; size_t bytes = 0; };
    std::vector<UnionTable> union_table;      // [id]; p null: the set's own staged bytes are in the union's form
    std::vector<uint8_t> slot_raw;
    lt::RawSetEntry* d_raw_sets = nullptr;
    uint16_t* d_unit_gain = nullptr;
    lt::RawUnion raw_union;
    int last_raw_walk_form = -1;              // lt_last_raw_walk_form
    // The device scratch of lt_raw_stats: the zone sums, histograms and zone counts of the call's slots, allocated by the first call (grown by
    // one that needs more), freed with the context.
    uint8_t* d_stats = nullptr;
    size_t stats_bytes = 0;
    // Input frames of another size (lt_set_input_size): src_w x src_h RGB frames, resized on the device to the calibration's size
    // (cv2.resize, INTER_LINEAR).  Per slot a staging frame of src_bytes = src_h * src_w * 3 bytes, src_stride apart (a multiple of 16
    // with at least 16 bytes of padding behind every frame: k_resize_rows reads aligned dwords); the uploads copy source rows into it
    // and k_resize_rows fills the rows of the slot's RGB camera frame, which everything else reads as in a plain context.  The tap
    // tables are built when the size is set: rs_yt on the host too (which source rows a run of rows reads).
    int src_w = 0, src_h = 0;                 // 0: frames of the calibration's size
    uint8_t* d_src = nullptr;
    size_t src_bytes = 0, src_stride = 0;
    uint32_t* d_rs_xt = nullptr;              // [img_w rounded up to 4][2] (resize_arith.h: pack_column)
    int32_t* d_rs_yt = nullptr;               // [img_h][4]
    std::vector<int32_t> rs_yt;
    // Frames in the caller's device memory (lt_attach_device_frames): the surface table -- one entry per slot, read by the table form
    // of the undistortion (k_frontend.hip) -- its host mirror (what lt_device_frames_rest passes on as kernel arguments) and which
    // slots are attached.  Allocated by the first attach; any upload of camera rows into a slot detaches it.
    lt::SurfEntry* d_surf = nullptr;
    std::vector<lt::SurfEntry> surf;
    std::vector<uint8_t> attached;
    // per slot: lt_overlay_run_inplace has drawn into the surface that was attached -- it holds no camera frame any more, and the slot
    // none of its own.  The planes of its front end are still the original pixels' (lt_mask_rerun works); a front end over it is
    // refused until an attach or an upload brings a frame.
    std::vector<uint8_t> drawn;
    uint32_t* d_und = nullptr;        // undistorted camera rows [r0, r0+nrows), one RGBX dword per pixel, slots 2p / 2p+1 interleaved (und_slot_base)
    size_t und_px = 0;                // pixels per slot of d_und
    lt::MaskArena masks;              // the mask chain's device memory, one block of each kind for the whole capacity
    lt::VizRing viz;                  // lt_search_viz_run / lt_split_panes_run: pictures on their way to the host
    int last_threshold_path = -1;                 // lt_last_threshold_path
    int last_tophat_path = -1;                    // lt_last_tophat_path
    int last_threshold_form = -1;                 // lt_last_threshold_form
    int last_open_form = -1;                      // lt_last_open_form
    int last_adaptive_path = -1;                  // 'neighborhood' calls: 1 = running box sums (k_adaptive_walk.hip), 0 = per-pixel windows
    int last_search_source = -1;                  // lt_last_search_source: 1 = the last search call read bit planes only, 0 = u8 masks
    // The walking threshold kernels are long serial walks (a wave covers half an image row or column): they win once a
    // call brings enough frames to fill the chip -- measured crossover 70-80 frames of 1100 x 1080 per call
    // (tools/threshold_crossover.py: 64 frames 232 vs 210 us, 96 frames 255 vs 304 us) -- and lose badly on a single
    // frame (164 vs 25 us).  Calls below this many pixels take the tile kernel.  LT_WALK_MIN_FRAMES=<n> (read at
    // lt_create, in frames of this context's bird's-eye size) overrides it; 0 = always walk.
    long long walk_min_pixels = 80LL * 1100 * 1080;
    // per slot: which forms of the mask are current.  The chain writes the bit plane only; the u8 mask
    // (d_plane[P_MASK]) is expanded from it when somebody asks for it; lt_upload_masks provides u8 only.
    std::vector<uint8_t> mask_bits_ok, mask_u8_ok;
    // per slot: the WHOLE camera frame is on the device (lt_upload_frames, or lt_upload_frame_rows + lt_upload_frame_rest; the row-run
    // uploads bring parts only) / the WHOLE annotated frame has been drawn (lt_overlay_run; the row-run and strip overlays draw
    // parts).  Whole-frame overlays and downloads refuse slots that are not (LT_ERR_STATE).
    std::vector<uint8_t> frame_full, annot_full;
    // per slot: the R / Lab-b planes (and the undistorted rows) are those of the camera rows the slot holds now -- set by lt_mask_run's
    // front end, cleared by every upload of camera rows and by lt_filter_run.  A second lt_mask_run over such slots with other
    // filter parameters (the second try of a frame, lane_tracker.py:1081-1101) skips the undistortion and the warp: same planes.
    std::vector<uint8_t> front_ok;
    lt_lane_record* d_rec = nullptr;
    double* d_prev = nullptr;
    uint32_t* d_pix = nullptr;
    int32_t* d_cent = nullptr;
    uint32_t* d_band_sums = nullptr;  // [slot][band][warp_w] column sums of the search bands
    // lt_search_fit_list: the item list, staged in page-locked memory and copied to the device ahead of its search; items_ev is
    // recorded behind the last kernel that reads the list (staging and device copy are written again only once it has fired)
    lt_search_item* d_items = nullptr;
    lt_search_item* h_items = nullptr;
    int items_cap = 0;
    hipEvent_t items_ev = nullptr;
    int maxpix = 0, maxlev = 0, maxbands = 0;
    bool have_mask = false;
    bool brute_tophat = false;
    // presentation stage (lt_overlay_*): inverse-warp table, per-slot row intervals, annotated frames
    int16_t* d_oxy = nullptr;
    uint16_t* d_ofrac = nullptr;
    bool have_overlay = false;
    int16_t* d_spans = nullptr;       // [slot][warp_h] (lo, hi)
    uint8_t* d_annot = nullptr;
    uint8_t* d_strip = nullptr;       // strip mode (lt_overlay_run_strip): rows [ov_r0, ov_r1) of every slot's annotated frame, packed
    size_t strip_bytes = 0;
    // Page-locked staging with one region PER SLOT (row intervals, text lines, glyph positions), so that an overlay call only
    // enqueues copies and kernels: calls over disjoint slots never wait for each other (the stream pipeline renders a window
    // in pieces while later frames are still searched).  A call over slots whose previous overlay may still be in flight
    // waits for that one first (overlay_lo / overlay_hi / overlay_done).
    int16_t* h_spans = nullptr;       // [capacity][warp_h * 2]
    int h_spans_cap = 0;
    struct StagingBusy { int lo = 0, hi = 0; hipEvent_t done = nullptr; };   // slots whose staging region a copy may still read
    StagingBusy spans_busy, text_busy;
    hipStream_t dl = nullptr;         // lt_download_overlay_async: device-to-host copies beside the compute and upload streams
    // The presentation kernels (spans copy, lane overlay, text) run on a stream of their own: on a slot's compute stream they would
    // queue behind the mask launches of LATER frames, which wait for uploads the bus has not delivered yet (measured: the first
    // overlay of a stream of windows ran 30 ms after its frames were ready).  It waits, per slot range, for the kernels that
    // wrote the slots' masks (hence for their camera rows) and for the copies of the remaining rows.
    hipStream_t present = nullptr;
    // lt_present_lane_from_fit_async: the plot rows (ploty, ploty ** 2) the device evaluates the averaged curves at, as last sent
    double* d_ploty = nullptr;        // [2][ploty_rows]
    std::vector<double> h_ploty;      // what d_ploty holds (compared on every call: 2 x 9 KB)
    hipStream_t lane_spec_stream = nullptr;   // the stream a speculative overlay of process() runs on, until lt_present_finish has waited for it
    unsigned lane_spec_ticket = 0;            // ... and the ticket a one-thread launch behind it stores at h_rec + 128 bytes (0: none, wait for the stream)
    // lt_set_urgent: while on, the stage calls run on this stream instead of the slots' streams -- behind what was enqueued
    // for THEIR slots only (slot-range events), not behind the masks of later frames queued on the slots' streams, which
    // wait for uploads still on the bus.  The stateful stream handles a frame whose first try failed this way.
    hipStream_t urgent = nullptr;
    bool urgent_on = false;
    StagingBusy annot_busy;           // annotated frames a copy on `dl` may still read
    // How the annotated frames go back (lt_download_overlay_async): by the copy engine or by a kernel that stores into the
    // page-locked destination.  Both are timed, copy by copy, with an event pair on the download stream; see choose_download().
    struct DlTimed { hipEvent_t a, b; double bytes; int method; };
    std::vector<DlTimed> dl_inflight;
    std::vector<hipEvent_t> dl_event_pool;
    double dl_rate[2] = {0.0, 0.0};   // GB/s, running mean of the last copies: [0] engine, [1] kernel
    int dl_samples[2] = {0, 0};
    int dl_method = 0;                // what the next copy uses
    int dl_since_probe = 0;           // copies since the other method was last tried
    int dl_forced = -1;               // LT_DL_KERNEL=0 / 1, lt_set_download_method: -1 = choose by measurement
    hipEvent_t rest_done = nullptr;   // end of the most recent lt_upload_frame_rest on the copy stream
    hipEvent_t store_done = nullptr;  // behind the most recent lt_overlay_store_device on the presentation stream (lt_overlay_store_wait)
    bool store_pending = false;
    bool rest_pending = false;
    // text: glyph atlas (set once) and the per-slot lines of the current call
    uint8_t *d_atlas = nullptr, *d_advance = nullptr, *d_lines = nullptr;
    int16_t* d_xpos = nullptr;
    std::vector<uint8_t> h_advance;
    uint8_t* h_lines = nullptr;       // page-locked, [text_slots][text_per_slot]
    int16_t* h_xpos = nullptr;
    int font_first = 0, font_glyphs = 0, font_gw = 0, font_gh = 0;
    size_t text_per_slot = 0;         // characters per slot the text buffers hold (n_lines * line_len of the largest call)
    int text_slots = 0;
    // ordering events of lt_upload_frame_rows_async (a ring: an event is reused long after its waits were enqueued)
    std::vector<hipEvent_t> order_events;
    size_t order_next = 0;
    // Slot-range bookkeeping of work in flight on the slots' streams, so that other streams wait for exactly what they
    // depend on instead of for the tails of those streams:
    //   readers -- kernels that READ the camera frames (undistortion, overlay): a stream-ordered upload into slots waits for
    //              the readers of those slots only, so the rows of later frames cross the bus while earlier ones are processed;
    //   writers -- kernels that wrote masks / records: a chained search waits for the writers of its own slots only.
    // A ring each; finished entries are dropped as new ones arrive (a long stream never synchronises the whole context).
    // The ring grows with the launches in flight (an outage group adds two or three entries per piece while the head
    // still waits for the bus); beyond 4096 entries it gives up (`overflow`) and waiters fall back to the tails of every
    // stream that can touch the slots, until the next full synchronisation.
    struct RangeEvents {
        struct Entry { int lo, hi; hipEvent_t ev; };
        std::vector<Entry> e = std::vector<Entry>(32, Entry{0, 0, nullptr});
        unsigned head = 0, count = 0;
        bool overflow = false;
        // work on the slots' streams that was NOT given an event of its own (note_range_frame: the one-frame calls of a context of
        // one or two slots -- LaneTracker.process() -- where every kernel of a frame runs on one stream and an event record between
        // two of them costs the frame ~6 us of device time each: profiles/r06_process_timeline.txt).  A waiter on another stream
        // then waits for the tails of the slots' streams, as after an overflow; cleared by the next full synchronisation.
        bool lazy = false;
        // ... and how much of it the HOST has seen finished: every lazy note counts (`lazy_seq`); a completion word the host polls
        // (lt_present_finish: the word stored behind the frame's overlay) carries the count at its launch, and seeing it moves
        // `lazy_seen` there -- everything noted up to then ran in front of it on the same stream.  lazy_seq == lazy_seen: nothing
        // unrecorded is in flight (the direct upload's question, lt_upload_frame_rows_enqueue).
        unsigned long long lazy_seq = 0, lazy_seen = 0;
        void reset() { head = count = 0; overflow = false; lazy = false; lazy_seen = lazy_seq; }
    };
    RangeEvents readers, writers;
    RangeEvents yuv_rows;                     // 4:2:0 / input-size context: the enqueued copies of source rows into staging (slots' streams): the conversion / resize of a slot's other rows waits for them
    RangeEvents rests;                        // lt_upload_frame_rest copies (copy stream): the overlay of a slot waits for ITS rows only
    // The chained band search of a stream (lt_band_fit_chain_run) is one workgroup walking many frames: it runs on a stream
    // of its own, beside the mask chains of later frames on the slots' streams.  A chain leaves its records in page-locked
    // host memory behind an event (lt_band_fit_chain_collect waits for that event only, not for the device).  Work on the
    // slots' streams that touches slots of a chain still in flight waits for it (for_each_slice).
    hipStream_t search = nullptr;
    int search_cus = 0;                       // lt_set_search_cus: CUs the search stream has to itself (0: none reserved)
    struct ChainTicket { int first, n; hipEvent_t done; int own; };   // own: first slot the chain searched itself (first + 1 when slot `first` is only its seed record)
    std::vector<ChainTicket> chains;          // not yet collected, oldest first
    std::vector<hipEvent_t> chain_event_pool;
    int* h_cancel = nullptr;                  // page-locked, device-visible: chains launched with an older epoch stop at their next frame
    int* d_cancel = nullptr;                  // its device address
    uint8_t* h_small = nullptr;               // page-locked scratch of the small downloads (download())
    uint8_t* h_lists = nullptr;               // page-locked landing area of lt_download_lane_lists (record + list region + centroids)
    size_t h_lists_bytes = 0;
    int ov_r0 = 0, ov_r1 = 0;                 // camera rows the lane overlay can change (lt_overlay_configure)
    lt_lane_record* h_rec = nullptr;          // page-locked mirror of the record of the last ONE-frame search (mirror_record)
    int rec_mirror_slot = -1;                 // the slot whose record the mirror holds once rec_mirror_stream is idle; -1: none
    hipStream_t rec_mirror_stream = nullptr;
    // the kernel that fills the mirror stores this ticket behind the record (k_band_chain3): lt_download_records polls for it
    // instead of waiting for the stream (0: the mirror is filled by a copy launch, wait for the stream)
    unsigned rec_ticket = 0, rec_ticket_counter = 0;
    lt_lane_record* h_rec_stage = nullptr;    // capacity records
    int h_rec_stage_cap = 0;
    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool stage_timing = false;
    std::vector<hipEvent_t> ev_pool;
    struct Pending { int stage; hipEvent_t a, b; };
    std::vector<Pending> pending;
    size_t ev_used = 0;
    float stage_ms[LT_NUM_STAGES] = {};
    int32_t stage_launches[LT_NUM_STAGES] = {};
};

namespace lt {

// ---- per-slot addresses in the context's buffers ------------------------------------------------------
inline uint8_t* slot_frame(const lt_ctx* c, int s) { return c->d_frames + (size_t)s * c->frame_bytes; }
// What a layout is, by name and never by comparison of its number: the RGB family's other members (BGR, RGBA, BGRA: a channel
// permutation of RGB, no coefficients), and the bytes a pixel of the layouts that are ONE plane of whole pixels (0 for 4:2:0).
inline bool is_rgb_family(int layout) { return layout == LT_INPUT_BGR || layout == LT_INPUT_RGBA || layout == LT_INPUT_BGRA; }
// 8-bit raw Bayer (RGGB, GRBG, GBRG, BGGR): one plane of one byte a pixel, an input format only
inline bool is_bayer(int layout) { return layout >= LT_INPUT_BAYER_RGGB && layout <= LT_INPUT_BAYER_BGGR; }
// 10- / 12-bit raw Bayer (layouts 32 .. 35, 48 .. 51: one plane of one 16-bit word a pixel; 36 .. 39, 52 .. 55: the same samples MIPI-packed),
// always behind a table; its sample bits
inline int raw_bits(int layout) { return raw_wide_bits(layout); }
inline bool is_bayer_wide(int layout) { return raw_bits(layout) != 0; }
// ... MIPI-packed (layouts 36 .. 39, 52 .. 55: one plane of bytes, five for four samples / three for two): the packing (mipi_arith.h: 0 RAW10,
// 1 RAW12), -1 for every other layout.  Their bits are raw_bits' 10 / 12: what is about the table holds for them as it is
inline int raw_packing(int layout) { return raw_pack(layout); }
// any raw mosaic, whatever its samples: what is about the mosaic (sizes, row runs, input only) and not about bytes
inline bool is_raw_mosaic(int layout) { return is_bayer(layout) || is_bayer_wide(layout); }
// what the front end and the row conversion of `c` are launched with (raw_setup.h)
// of raw set `id` (0: the context's own, which is what everything that has no slot -- the one-shot converters -- keeps)
inline int raw_set_count(const lt_ctx* c) { return 1 + (int)c->raw_more.size(); }
inline const RawSetup& raw_set_of(const lt_ctx* c, int id) { return id > 0 ? c->raw_more[(size_t)id - 1].s : c->raw; }
inline const RawDevice& raw_dev_of(const lt_ctx* c, int id) { return id > 0 ? c->raw_more[(size_t)id - 1].d : c->raw_dev; }
inline RawStages raw_stages_of(const lt_ctx* c, int id = 0) { return raw_stages(raw_set_of(c, id), raw_dev_of(c, id)); }
inline int slot_raw_set(const lt_ctx* c, int s) { return s >= 0 && s < (int)c->slot_raw.size() ? c->slot_raw[(size_t)s] : 0; }
// How the raw kernels of a launch over slots [first, first + n) find their stages: all slots one set -- `ids` null, `one` that set's stages,
// today's kernels -- or several sets: `one` says which kernel (the union's stages), sets / ids (one byte per slot, host memory) what each slot reads.
struct RawRun {
    RawStages one;
    const RawSetEntry* sets = nullptr;
    const uint8_t* ids = nullptr;
};
inline RawRun raw_run_of(const lt_ctx* c, int first, int n) {
    RawRun r;
    const int id0 = slot_raw_set(c, first);
    bool mixed = false;
    for (int i = first + 1; i < first + n && !mixed; ++i) mixed = slot_raw_set(c, i) != id0;
    if (!mixed || !c->raw_union.staged || !c->d_raw_sets) {       // (sets that stage nothing differ in nothing a kernel reads)
        r.one = raw_stages_of(c, mixed ? 0 : id0);
        return r;
    }
    r.one = raw_union_stages(c->in_layout, c->raw_union, c->d_raw_sets);
    r.sets = c->d_raw_sets, r.ids = &c->slot_raw[(size_t)first];
    return r;
}
inline int packed_bpp(int layout) {
    return layout == LT_INPUT_RGB || layout == LT_INPUT_BGR ? 3 : layout == LT_INPUT_RGBA || layout == LT_INPUT_BGRA ? 4
           : layout == LT_INPUT_YUY2 || layout == LT_INPUT_UYVY || (is_bayer_wide(layout) && raw_packing(layout) < 0) ? 2 : is_bayer(layout) ? 1 : 0;
}
// the bytes of a row of w pixels of the layouts that are ONE plane (0 for 4:2:0): whole pixels, or packed 10- / 12-bit samples -- what every
// place that sizes or checks a frame from its layout asks
inline int one_plane_row_bytes(int layout, int w) { return raw_packing(layout) >= 0 ? raw_wide_row_bytes(layout, w) : packed_bpp(layout) * w; }
inline uint8_t* slot_yuv(const lt_ctx* c, int s) { return c->d_yuv + (size_t)s * c->yuv_stride; }
inline uint8_t* slot_src(const lt_ctx* c, int s) { return c->d_src + (size_t)s * c->src_stride; }
inline bool resizes(const lt_ctx* c) { return c->src_w > 0; }   // the caller's frames have another size (lt_set_input_size)
inline YuvCoef yuv_coef_of(const lt_ctx* c) { return YuvCoef{c->yuv_coef[0], c->yuv_coef[1], c->yuv_coef[2], c->yuv_coef[3], c->yuv_coef[4]}; }
inline uint8_t* slot_mask(const lt_ctx* c, int s) { return c->masks.d_plane[P_MASK] + (size_t)s * c->masks.plane_bytes; }
// the opened bit plane of slot s as the searches take it; use_bits = false: none (they read slot_mask)
inline MaskBits slot_bits(const lt_ctx* c, int s, bool use_bits) {
    return MaskBits{use_bits ? c->masks.d_bits_open + (size_t)s * c->masks.bits_stride : nullptr, c->masks.bits_stride, (c->calib.warp_w + 63) / 64};
}
inline lt_lane_record* slot_rec(const lt_ctx* c, int s) { return c->d_rec + s; }
inline double* slot_prev(const lt_ctx* c, int s) { return c->d_prev + (size_t)s * 6; }
inline uint32_t* slot_pix(const lt_ctx* c, int s) { return c->d_pix + (size_t)s * 2 * c->maxpix; }           // [side][maxpix]
inline int32_t* slot_cent(const lt_ctx* c, int s) { return c->d_cent + (size_t)s * 2 * (c->maxlev + 2); }    // [side][maxlev + 2]
inline uint32_t* slot_band_sums(const lt_ctx* c, int s, int nbands) { return c->d_band_sums + (size_t)s * nbands * c->calib.warp_w; }

// ---- calibration sets (lt_api.cpp) ------------------------------------------------------------------------------
inline int slot_set(const lt_ctx* c, int s) { return s >= 0 && s < (int)c->slot_cal.size() ? c->slot_cal[(size_t)s] : 0; }
// the first slot of [first, first + n) whose set is not 0, or -1: what the entry points that know set 0's tables only ask
inline int first_foreign(const lt_ctx* c, int first, int n) {
    for (int i = first; i < first + n; ++i)
        if (slot_set(c, i) != 0) return i;
    return -1;
}
int refuse_foreign(lt_ctx* c, int first, int n, const char* who);   // LT_ERR_STATE if one of the slots has another set than 0
bool union_rows(lt_ctx* c);                                         // fe.r0 / fe.nrows, cam_r0 / cam_r1, ov_r0 / ov_r1 := the unions over the sets
void refresh_cal0(lt_ctx* c);                                       // cal[0] := the context's own tables and rows

// ---- raw Bayer conditioning, one-shot conversion (lt_raw.cpp) ----------------------------------------------------
// `s` onto the device, for a context or for one call -- the only code that allocates or writes either buffer of `d`: the table buffer :=
// raw_staged(s), and -- new_map -- the gain plane := the mesh expanded on `st` for frames of h x w (the host waits); no map: no plane.  An error
// with nothing written leaves `d` as it was; a failed expansion has taken the map out of `s` AND `d` (better none than one they disagree on).
int raw_commit(RawSetup& s, RawDevice& d, bool new_map, hipStream_t st, int h, int w);
void raw_release(RawDevice& d);
void raw_sets_release(lt_ctx* c);                                   // sets 1 .., the set table, the union forms, the plane of unit gains (lt_destroy)
int ensure_cal_table(lt_ctx* c);                                    // lt_api.cpp: d_cal exists and holds set 0 (the set-per-slot raw forms read it)
// before a launch that may mix raw sets: the set table is there (a failed rewrite took it away) and so is the calibrations' table
inline int raw_sets_ready(lt_ctx* c) {
    if (c->raw_more.empty()) return LT_OK;
    if (!c->d_raw_sets) return fail(LT_ERR_STATE, "the table of raw sets could not be written when a set last changed: set one again");
    return ensure_cal_table(c);
}
// lt_set_input_format: a raw table stays with 8-bit Bayer, stage and map go, a wide layout has its default staged -- before anything else changes
int raw_take_layout(lt_ctx* c, int layout);
int check_raw_size(int layout, int h, int w);                       // a frame of a raw layout: even sides from 4, RAW10 rows whole groups
int check_one_shot_size(int layout, int h, int w);                  // ... and of a one-shot converter, any layout: at most 16384 a side
// one host frame in raw.layout (any but RGB) -> RGB on the device, behind `raw` where that is a raw layout (committed here, for the call)
int convert_once(lt_ctx* c, const char* what, const void* frame, size_t in_bytes, int h, int w, YuvCoef k, RawSetup raw, uint8_t* out_rgb);

// ---- LT_TRACE_START=1 (lt_memory.cpp): one line per set-up phase on stderr -------------------------------
//   lt_start <seconds on CLOCK_MONOTONIC, = Python's time.monotonic()> <what> <ms> [<bytes>]
// What a first window of a stream or the first calls of process() spend outside the kernels: context growth (lt_reserve,
// hipMalloc, cache hits and misses), page-locked allocations, table builds and uploads.  tools/cold_start.py reads them.
bool trace_on();
double trace_now();                                          // seconds, CLOCK_MONOTONIC
void trace_line(const char* what, double t0, size_t bytes = 0);   // prints the phase that started at t0 (trace_now())
struct TraceScope {
    const char* what;
    size_t bytes;
    double t0;
    TraceScope(const char* w, size_t b = 0) : what(w), bytes(b), t0(trace_on() ? trace_now() : 0.0) {}
    ~TraceScope() { if (trace_on()) trace_line(what, t0, bytes); }
};

// ---- host copy threads, staging blocks (lt_memory.cpp), for lt_present.cpp ----------------------------------
int host_submit_copy2d(int group, uint8_t* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t width, size_t height,
                       std::shared_ptr<void> hold);          // `hold` is released when the last piece of the copy has run
int host_submit_fn(int group, std::function<void()> fn, bool many);
int host_reserve(int group);                                 // a piece that will be submitted later: the group waits for it
void host_unreserve(int group);
void host_after_event(hipEvent_t ev, int device, std::function<void()> then);   // `then` runs on the library's waiter thread once `ev` has fired
int host_copy_threads();
int host_copy_pollers();                                     // copy threads polling for work right now (they take a piece within a microsecond)
void* pinned_block_acquire(size_t bytes);                    // page-locked staging, pooled per size (nullptr: allocation failed)
void pinned_block_release(void* p, size_t bytes);
hipEvent_t pooled_event();                                   // process-wide events (they outlive the context that recorded them)
void pooled_event_release(hipEvent_t e);

// ---- device memory (lt_memory.cpp): a cache in front of hipMalloc / hipFree ------------------------------
void* cached_alloc(size_t bytes);
void cached_free(void* p);
// the block the cache has handed out that holds address p (lt_device_alloc's blocks, the contexts' own buffers): its base, size and device
bool cached_block_find(const void* p, const void** base, size_t* bytes, int* device);
// Frees of one thread bracketed by this wait for `device` ONCE and enter the cache together when the scope closes -- behind
// the allocations made inside it (lt_reserve: the larger blocks first, then the old ones into the cache; lt_destroy).
struct FreeScope {
    explicit FreeScope(int device);
    ~FreeScope();
    FreeScope(const FreeScope&) = delete;
    FreeScope& operator=(const FreeScope&) = delete;
};

template <class T>
int dev_alloc(T** p, size_t count) {
    if (count == 0) count = 1;
    *p = static_cast<T*>(cached_alloc(count * sizeof(T)));
    if (!*p) return fail(LT_ERR_NOMEM, "hipMalloc(%zu bytes) failed", count * sizeof(T));
    return LT_OK;
}
template <class T>
void dev_free(T*& p) {
    if (p) cached_free(p);
    p = nullptr;
}
// a device buffer of one call: freed when its scope closes, on every path
template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { dev_free(p); }
    int alloc(size_t count) { return dev_alloc(&p, count); }
};

// ---- the mask chain's arena (MaskArena, above) ----------------------------------------------------------------
inline void MaskArena::set_geometry(int h, int w) {
    plane_bytes = (size_t)h * w;
    bits_stride = (size_t)h * ((w + 63) / 64);
    th_pitch = (w + 63) & ~63;
    th_pad_bytes = (size_t)h * th_pitch;
    zone_stride = (size_t)((w + 127) / 128) * tophat_split_zone_dwords(55);
}

inline int MaskArena::reserve(int slots, bool batch) {
    release();
    capacity = slots;
    const size_t n = (size_t)slots;
    int rc;
    for (int i : {(int)P_R, (int)P_B, (int)P_THR, (int)P_THB, (int)P_T0})
        if ((rc = dev_alloc(&d_plane[i], n * plane_bytes))) return rc;
    for (auto q : {&d_bits_merged, &d_bits_eroded})
        if ((rc = dev_alloc(q, n * bits_stride))) return rc;
    if (!batch) return LT_OK;
    for (auto q : {&d_bits_open, &d_bits_tmp, &d_bits_tmp2})
        if ((rc = dev_alloc(q, n * bits_stride))) return rc;
    for (auto& q : d_th_pad)
        if ((rc = dev_alloc(&q, n * th_pad_bytes))) return rc;
    th_padded.assign(n, 0);
    return LT_OK;
}

inline void MaskArena::release() {
    for (auto& q : d_plane) dev_free(q);
    for (auto q : {&d_bits_merged, &d_bits_eroded, &d_bits_open, &d_bits_tmp, &d_bits_tmp2, &d_bits_n1, &d_bits_n2}) dev_free(*q);
    for (auto q : {&d_th_pad[0], &d_th_pad[1], &d_b_pad, &d_side_scratch}) dev_free(*q);
    dev_free(d_zone);
    th_padded.clear();
    capacity = 0;
}

// Planes only some paths use are allocated when one of those paths runs first (the whole capacity at once): the u8 mask
// (d_plane[P_MASK]: lt_upload_masks, lt_download_masks, searches outside the bit-plane kernels' limits), the expanded merged
// plane (lt_download_plane), the scratch planes of the older threshold kernels (P_T1 .. P_T3).  A 768-slot context is 10.4 GB
// instead of 14.6 -- and device memory that has been used before costs ~16 ms per GB to allocate (the driver clears it: NOTES D.2).
inline int MaskArena::ensure_plane(int idx) {
    return d_plane[idx] ? (int)LT_OK : dev_alloc(&d_plane[idx], (size_t)capacity * plane_bytes);
}

inline int MaskArena::ensure_noise_buffers() {
    const size_t n = (size_t)capacity;
    int rc;
    if (!d_b_pad && (rc = dev_alloc(&d_b_pad, n * th_pad_bytes))) return rc;
    if (!d_bits_n1 && (rc = dev_alloc(&d_bits_n1, n * bits_stride))) return rc;
    if (!d_bits_n2 && (rc = dev_alloc(&d_bits_n2, n * bits_stride))) return rc;
    return LT_OK;
}

// (per STREAM, not per slot: a context of a thousand slots runs its one- and two-frame calls on a handful of streams -- the
// slices' streams and the urgent one -- and calls on one stream are ordered)
inline int MaskArena::ensure_side_scratch() {
    return d_side_scratch ? (int)LT_OK : dev_alloc(&d_side_scratch, (size_t)SIDE_LANES * 2 * plane_bytes);
}

// (per SLOT, like the scratch plane P_T0: slots of different slices are in flight at once.  Never written by the host and never
// read before the same launch wrote it, so it is not cleared.)
inline int MaskArena::ensure_zone_scratch() {
    return d_zone ? (int)LT_OK : dev_alloc(&d_zone, (size_t)capacity * zone_stride * sizeof(uint32_t));
}

// ---- streams, slot ranges, ordering (lt_api.cpp) ---------------------------------------------------------
int sync_all(lt_ctx* c);
int note_range(lt_ctx::RangeEvents& r, hipStream_t st, int lo, int hi);
int note_range_frame(lt_ctx* c, lt_ctx::RangeEvents& r, hipStream_t st, int lo, int hi);   // ... without an event where the context is one frame's (RangeEvents::lazy)
int wait_range(const lt_ctx::RangeEvents& r, hipStream_t waiter, int lo, int hi, bool* precise);
int note_written(lt_ctx* c, hipStream_t st, int lo, int hi);
hipEvent_t next_order_event(lt_ctx* c);
int wait_tail(lt_ctx* c, hipStream_t waiter, hipStream_t st);   // `waiter` waits for what is enqueued on `st` so far (an order event)
int wait_chains(lt_ctx* c, hipStream_t st, int lo, int hi);
int flush_stage_events(lt_ctx* c);
int check_slots(lt_ctx* c, int first, int n);
int set_device(lt_ctx* c);
hipError_t create_compute_stream(hipStream_t* st, int reserved = 0);
// (stream_get / stream_put -- the per-process stream pool -- are declared in lt_internal.h)
int download(lt_ctx* c, const void* src, void* dst, size_t bytes);
int ensure_bev(lt_ctx* c);
int ensure_search_buffers(lt_ctx* c, int maxpix, int maxlev);
bool masks_have_bits(const lt_ctx* c, int first, int n);
int ensure_u8_masks(lt_ctx* c, int first, int n);
int make_search_geom(lt_ctx* c, const lt_search_params* p, bool band, SearchGeom& g);
int ensure_band_sums(lt_ctx* c, int nbands);
int prepare_search(lt_ctx* c, const lt_search_params* p, bool band, SearchGeom& g);
bool slot_reads_bits(const lt_ctx* c, const SearchGeom& g, int mode, int first, int n);
void mark_frames(lt_ctx* c, int first, int n, int full);
void front_stale(lt_ctx* c, int first, int n);                  // new camera rows in these slots: their planes are the old frames'
void detach_slots(lt_ctx* c, int first, int n);                 // an upload into these slots: their front end reads the slots' own frames again
int wait_camera_readers(lt_ctx* c, hipStream_t st, int first, int n);   // `st` waits for the kernels that still read the camera rows of these slots
int wait_reader_tails(lt_ctx* c, hipStream_t waiter);           // ... for the tail of every stream such a kernel can be on
void mark_annot(lt_ctx* c, int first, int n, int full);
int first_partial(const std::vector<uint8_t>& v, int first, int n);
// A plane of a caller's surface, checked on the host before anything is launched (lt_attach_device_frames, the device sinks): device
// memory of `device`, known to this runtime, its whole extent inside one allocation.  `memo`: the allocation the runtime was last
// asked about, within one call.
struct KnownRange { uintptr_t base = 0; size_t size = 0; };
int check_plane(int device, const void* p, size_t extent, int k, int i, KnownRange& memo);
// device sinks (lt_sink.cpp), shared with lt_overlay_run_to_surfaces: the layout, size and coefficients of a sink; then every plane
// of the n destinations through check_plane's rules, no two planes sharing a byte, none sharing a byte with a camera surface attached
// to a slot of the context -> the kernels' entries
int check_sink_format(int layout, int h, int w, const int32_t* coeffs);
int check_ctx_sinks(lt_ctx* c, const lt_device_surface* dst, int n, int layout, std::vector<SurfEntry>& ent);
int ensure_search_stream(lt_ctx* c);                          // lt_chain.cpp
int ensure_chain_buffers(lt_ctx* c);                          // lt_chain.cpp
int warm_presentation(lt_ctx* c, bool strips);                // lt_present.cpp
int warm_search_viz(lt_ctx* c, bool panes);                   // lt_search_viz.cpp: the staging ring (lt_warm)
void viz_free_device(lt_ctx* c);                              // lt_search_viz.cpp: the ring's device memory (free_slots)
void viz_free_host(lt_ctx* c);                                // ... its events and page-locked staging (lt_destroy)




// Slot -> stream mapping is fixed (contiguous slices of the capacity), so consecutive stages of one
// slot stay ordered on one stream while different slices overlap: the latency-bound search of one
// slice runs under the mask chain of another.  Slice si of k holds slots [lo, hi) and runs on streams[si].
inline int slice_count(const lt_ctx* c) { return std::max(1, std::min(c->nstreams, c->capacity)); }
inline void slice_bounds(const lt_ctx* c, int si, int k, int* lo, int* hi) {
    // even boundaries: the undistorted rows of slots 2p and 2p+1 are interleaved, and the warp serves a pair with one load
    *lo = (int)((long long)c->capacity * si / k) & ~1;
    *hi = si + 1 == k ? c->capacity : (int)((long long)c->capacity * (si + 1) / k) & ~1;
}
inline int slice_of(const lt_ctx* c, int slot) {
    const int k = slice_count(c);
    for (int si = 0; si < k; ++si) {
        int lo, hi;
        slice_bounds(c, si, k, &lo, &hi);
        if (slot < hi) return si;
    }
    return k - 1;
}

// Calls fn(stream, first, n) for every non-empty piece of slots [first, first + n).
template <class F>
int for_each_slice(lt_ctx* c, int first, int n, F fn) {
    const int k = slice_count(c);
    if (c->urgent_on && c->urgent) {
        // one piece on the urgent stream: behind the kernels that wrote these slots (or, with the ring overflowed, the tails of
        // their streams) and a chain still touching them; the slots' own streams then wait for it, so that whatever is
        // enqueued for these slots later stays ordered behind it
        hipStream_t us = c->urgent;
        bool precise = true;
        int rc = wait_range(c->writers, us, first, first + n, &precise);
        if (rc) return rc;
        auto slices = [&](auto g) {
            for (int si = 0; si < k; ++si) {
                int lo, hi;
                slice_bounds(c, si, k, &lo, &hi);
                if (std::min(first + n, hi) > std::max(first, lo)) { int r = g(c->streams[si]); if (r) return r; }
            }
            return (int)LT_OK;
        };
        if (!precise && (rc = slices([&](hipStream_t st) { return wait_tail(c, us, st); }))) return rc;
        if ((rc = wait_chains(c, us, first, first + n))) return rc;
        if ((rc = fn(us, first, n))) return rc;
        hipEvent_t done = next_order_event(c);
        if (!done) return fail(LT_ERR_HIP, "hipEventCreate failed");
        HIP_TRY(hipEventRecord(done, us));
        return slices([&](hipStream_t st) {
            HIP_TRY(hipStreamWaitEvent(st, done, 0));
            return (int)LT_OK;
        });
    }
    for (int si = 0; si < k; ++si) {
        int lo, hi;
        slice_bounds(c, si, k, &lo, &hi);
        const int a = std::max(first, lo), b = std::min(first + n, hi);
        if (b <= a) continue;
        int rc = wait_chains(c, c->streams[si], a, b);                     // a chain in flight reads / writes these slots
        if (rc) return rc;
        rc = fn(c->streams[si], a, b - a);
        if (rc) return rc;
    }
    return LT_OK;
}

// RAII-free helper pair: bracket one kernel launch with events when stage timing is on (c = nullptr: no timing sink, does nothing)
struct StageScope {
    lt_ctx* c;
    int stage;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    StageScope(lt_ctx* c_, int stage_, hipStream_t st_ = nullptr) : c(c_), stage(stage_), st(st_ || !c_ ? st_ : c_->stream) {
        if (!c || !c->stage_timing) return;
        if (c->ev_used + 2 > c->ev_pool.size()) {
            if (flush_stage_events(c) != LT_OK) return;
            while (c->ev_pool.size() < 256) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) break;
                c->ev_pool.push_back(e);
            }
        }
        if (c->ev_used + 2 > c->ev_pool.size()) return;
        a = c->ev_pool[c->ev_used++];
        b = c->ev_pool[c->ev_used++];
        (void)hipEventRecord(a, st);
    }
    ~StageScope() {
        if (!a) return;
        (void)hipEventRecord(b, st);
        c->pending.push_back({stage, a, b});
    }
};

// ---- the mask chain (lt_mask_chain.cpp) -------------------------------------------------------------------
int validate_filter(const lt_filter_params* p);
// what the chain takes from a context besides the arena
struct ChainEnv {
    const EllipseSE *se29 = nullptr, *se55 = nullptr;   // the brute-force top-hats' footprints
    bool brute_tophat = false;
    long long walk_min_pixels = 0;                      // calls of fewer pixels take the tile kernels (lt_ctx::walk_min_pixels)
    const std::vector<hipStream_t>* streams = nullptr;  // whose position picks a stream's lane of the side scratch; null: the spare lane
    lt_ctx* timing = nullptr;                           // the context whose stage timers take the launches (StageScope); null: untimed
    int *threshold_path = nullptr, *adaptive_path = nullptr;   // lt_last_threshold_path / lt_last_adaptive_path; null: nobody asks
    int* tophat_path = nullptr;                         // lt_last_tophat_path; null: nobody asks
    int* threshold_form = nullptr;                      // lt_last_threshold_form; null: nobody asks
    int* open_form = nullptr;                           // lt_last_open_form; null: nobody asks
};
// filter_lane_points() (lane_tracker.py:210-238) on planes P_R / P_B of slots [first, first + n) of the arena, h x w pixels each, on
// stream s; call_frames: the frames of the whole call this piece belongs to.  The opened mask lands in d_bits_open, or with
// u8_mask in d_plane[P_MASK] (allocated here if need be).
int run_mask_chain(MaskArena& a, const ChainEnv& env, hipStream_t s, int first, int n, const lt_filter_params* p, int h, int w,
                   int call_frames, bool u8_mask = false);

}  // namespace lt
