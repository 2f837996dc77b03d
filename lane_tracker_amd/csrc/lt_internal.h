// Internal declarations shared by the C-ABI layer (lt_api.cpp, lt_mask_chain.cpp), the host table builders
// (lt_tables.cpp) and the kernel launchers (*.hip).  Not installed; the public ABI is
// include/lane_tracker_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include <cstdlib>

#include "../../include/lane_tracker_amd.h"
#include "raw_setup.h"
#include "yuv_arith.h"

// Measurement switches -- alternative kernels and launch shapes for A/B runs, each held bit-exact by the parity suite -- exist in
// the EXPERIMENTS build only (`make EXPERIMENTS=1` -> liblane_tracker_amd_exp.so, -DLT_EXPERIMENTS; tools/* and
// tests/test_gpu_parity.py::test_alternative_kernel_paths_keep_parity load that one).  In the release library LT_EXP_ENV(...) is a
// null pointer constant: the path behind a switch is dead code the compiler drops, and the switch's name does not reach the
// binary (tests/test_native_abi.py counts the LT_* strings of the release .so against INTEGRATION.md section E).
#ifdef LT_EXPERIMENTS
#define LT_EXP_ENV(name) std::getenv(name)
#else
#define LT_EXP_ENV(name) (static_cast<const char*>(nullptr))
#endif

namespace lt {

// ---- host tables (lt_tables.cpp) ----------------------------------------------------------------
struct RemapTable {              // cv::remap fixed-point maps: integer tap + 5+5-bit fraction
    std::vector<int16_t> xy;     // (sx, sy) interleaved
    std::vector<uint16_t> frac;  // fy*32 + fx
    int rows = 0, cols = 0;
};
void build_warp_table(const lt_calib& c, RemapTable& t);
void warp_source_rows(const lt_calib& c, const RemapTable& warp, int& r0, int& r1);
void build_undistort_table(const lt_calib& c, int r0, int r1, RemapTable& t);
void build_lab_tables(uint16_t gamma_tab[256], uint16_t cbrt_tab[3072], int32_t coeffs[9]);
int  ellipse_halfwidths(int k, int* dx);  // returns tap count

struct EllipseSE {               // one horizontal run per row
    int k;
    int8_t dx[64];
};

// ---- kernel launchers ----------------------------------------------------------------------------
struct FrontEndGeom {
    int img_h, img_w, warp_h, warp_w, r0, nrows;
};
// The undistorted rows of slots 2p and 2p+1 are interleaved per pixel (k_frontend.hip): dword index of pixel 0 of a slot;
// its pixel i is 2 i dwords further.  The buffer holds ceil(slots / 2) pairs of 2 * und_px dwords.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline size_t und_slot_base(size_t und_px, int slot) { return (size_t)(slot >> 1) * 2 * und_px + (size_t)(slot & 1); }
// `und` is the base of the whole buffer, `first_slot` the absolute slot of frame 0 of the call; planes point at that slot's data
void launch_warp_split(hipStream_t s, const uint32_t* und, size_t und_px, int first_slot, const int16_t* wxy,
                       const uint16_t* wfrac, FrontEndGeom g, const uint16_t* gamma_tab, const uint16_t* cbrt_tab,
                       const int32_t* coeffs, bool lab_clamp_dead, uint8_t* planeR, uint8_t* planeB, size_t plane_stride, int n);
// (YuvCoef, the five coefficients of the YUV 4:2:0 input's conversion: yuv_arith.h)
// (RawStages -- `raw`, here and below -- and raw_wide_bits, raw_pack, raw_wide_row_bytes, what the raw layouts' numbers say: raw_setup.h)
// mesh (device memory, uint16[4][mh][mw], phase-major) -> the gain plane of an h x w image whose layout has `pattern` (k_shade_expand)
void launch_shade_expand(hipStream_t s, const uint16_t* mesh, int mw, int mh, int pattern, uint16_t* plane, int h, int w);
// Raw Bayer statistics (lt_raw_stats; k_raw_stats.hip, stats_arith.h): histograms and zone sums of the samples of slots [first_slot,
// first_slot + n) as they enter the raw table, ADDED to hist / zone_count / zone_sum (device memory, zeroed by the caller; per slot 4 << bits
// (8 bits: 1024) / grid_h * grid_w / 4 * grid_h * grid_w values apart, the launch's first slot at the pointers).  The frames: src.tab -- the
// surface table, entries [first_slot, first_slot + n) -- or src.frames, the staging frame of first_slot, src.stride bytes a slot.  The
// rectangle is ncy x ncx cells of 2 x 2 sites from (row0, col0), all even and inside the frame; 1 <= grid_h <= min(64, ncy), likewise grid_w;
// lo / hi by phase; gains not null: the shading map's plane (RawStages::gains) and its pedestals blk.
struct RawStatsJob {
    int pattern, bits, pack;                 // layout & 3; 8, 10 or 12; raw_pack(layout)
    int img_w;
    int row0, col0, ncy, ncx, grid_h, grid_w;
    int32_t lo[4], hi[4];
    const uint16_t* gains = nullptr;
    RawShadeBlack blk = {};
    uint32_t *hist = nullptr, *zone_count = nullptr;
    unsigned long long* zone_sum = nullptr;
};
// rows [r0, r1) of n dense frames of h x w in `layout` (any but 0; the layouts: launch_undistort_rows) -> the same rows of n RGB frames
// (k_rows_to_rgb<layout, false, ..>; behind a raw table k_raw_rows_rgb<pattern, false, ..>)
void launch_yuv_rows_to_rgb(hipStream_t s, int layout, const uint8_t* yuv, size_t yuv_stride, YuvCoef k, uint8_t* rgb,
                            size_t rgb_stride, int h, int w, int r0, int r1, int n, const RawStages& raw = RawStages(),
                            const RawSetEntry* rsets = nullptr, const uint8_t* rids = nullptr);
// Input frames of another size (lt_set_input_size; k_resize.hip): destination rows [a, b) of n RGB frames of width w, dst_stride apart, :=
// cv2.resize(INTER_LINEAR) of n RGB staging frames of src_bytes (rows of src_w pixels), src_stride apart.  xt: two words per destination
// column (resize_arith.h: pack_column), padded to a multiple of four columns; yt: (tap0, tap1, c0, c1) per destination row; device memory.
void launch_resize_rows(hipStream_t s, const uint8_t* src, size_t src_stride, size_t src_bytes, int src_w, uint8_t* dst, size_t dst_stride,
                        int w, int a, int b, const uint32_t* xt, const int32_t* yt, int n);
// Frames in the caller's device memory (lt_attach_device_frames): one entry per slot of the context's surface table -- the plane
// pointers (RGB: [0]; NV12: Y, UV; I420: Y, U, V) and the row pitches of the luma / RGB plane and of the chroma plane(s), in bytes.
// Checked on the host before they reach a kernel: pitches at least a row and below 2^23 (24-bit multiplies), planes below 2^31 bytes.
struct SurfEntry {
    uint64_t plane[3];
    int32_t pitch, cpitch;
};
static_assert(sizeof(SurfEntry) == 32, "SurfEntry: 32 bytes, two scalar loads");
struct SurfChunk {               // the entries of one launch, by value
    static constexpr int N = 32;
    SurfEntry e[N];
};
// Where the undistortion finds the frames of slots [first_slot, first_slot + n): in the slots themselves -- `frames` = the frame
// of first_slot, `stride` bytes per slot: the RGB camera frames (8 bytes of padding behind each) or the 4:2:0 staging frames (a
// multiple of 16 apart, 16 bytes of padding behind the last) -- or on the caller's surfaces, entries [first_slot, first_slot + n)
// of `tab` (device memory).
struct FrameSource {
    const SurfEntry* tab;        // not null: surfaces
    const uint8_t* frames;
    size_t stride;
    static FrameSource slots(const uint8_t* frames, size_t stride) { return FrameSource{nullptr, frames, stride}; }
    static FrameSource surfaces(const SurfEntry* tab) { return FrameSource{tab, nullptr, 0}; }
};
void launch_raw_stats(hipStream_t s, FrameSource src, int first_slot, int n, const RawStatsJob& job);      // (RawStatsJob: above)
// the undistorted rows of n frames (layout 0 = RGB, 1 = NV12, 2 = I420, 3 = YUY2, 4 = UYVY, 5 = BGR, 6 = RGBA, 7 = BGRA, 16 .. 19 = raw Bayer RGGB /
// GRBG / GBRG / BGGR, 32 .. 35 / 48 .. 51 = the same at 10 / 12 bits, 36 .. 39 / 52 .. 55 = those MIPI-packed, which need raw.table; `k` is read for the YUV layouts only: every tap
// converted, then the same blend); `und` is the base of the whole buffer, `first_slot` the absolute slot of frame 0 of the call
// (k_undistort_rows<layout, source, false>; behind a raw table k_raw_walk_rows<pattern, source, false, stages>)
void launch_undistort_rows(hipStream_t s, FrameSource src, int layout, YuvCoef k, const int16_t* uxy, const uint16_t* ufrac,
                           FrontEndGeom g, uint32_t* und, size_t und_px, int first_slot, int n, const RawStages& raw = RawStages());
// Calibration sets (lt_add_calibration): the remap tables of one set as the table-per-slot front end finds them -- entry `id` of the
// context's set table (device memory, written when a set is added or rebuilt: before the context's first upload, with nothing in
// flight).  Which set a slot of a launch has travels BY VALUE, one byte per slot of the launch (id of slot first_slot + z: byte z):
// an assignment changes every tick of a group, and an argument cannot be rewritten under a launch still queued on another stream.
struct CalTables {
    const int16_t* uxy;
    const uint16_t* ufrac;
    const int16_t* wxy;
    const uint16_t* wfrac;
};
static_assert(sizeof(CalTables) == 32, "CalTables: 32 bytes, two scalar loads");
constexpr int LT_MAX_CALIBRATIONS = 256;   // an id is a byte
struct CalIds {                  // the sets of the slots of one launch
    static constexpr int N = 64;
    uint32_t w[N / 4];
};
// The table-per-slot forms of the two launches above, for slots [first_slot, first_slot + n) whose sets are ids[0, n) (host memory):
// every slot with the tables of its own set, one frame per walk; launches of up to CalIds::N slots (k_undistort_rows<layout, source, true>, k_warp_cal).
// rids not null: the raw sets of the slots, ids of entries of `rsets` (raw_setup.h: RawSetEntry) -- the set-per-slot forms of the raw walk,
// k_rawset_walk_rows / k_packset_walk_rows<pattern, source, stages>, `raw` saying which stages (those of the union of the sets) and nothing else;
// likewise below and above for the row conversions (k_rawset_rows_rgb / k_packset_rows_rgb), rids[z] the set of frame z of the launch.
void launch_undistort_cal(hipStream_t s, FrameSource src, int layout, YuvCoef k, const CalTables* sets, const uint8_t* ids,
                          FrontEndGeom g, uint32_t* und, size_t und_px, int first_slot, int n, const RawStages& raw = RawStages(),
                          const RawSetEntry* rsets = nullptr, const uint8_t* rids = nullptr);
void launch_warp_cal(hipStream_t s, const uint32_t* und, size_t und_px, int first_slot, const CalTables* sets, const uint8_t* ids,
                     FrontEndGeom g, const uint16_t* gamma_tab, const uint16_t* cbrt_tab, const int32_t* coeffs, uint8_t* planeR,
                     uint8_t* planeB, size_t plane_stride, int n);
// entries[0, n) (host memory, consumed before the call returns) -> tab[first, first + n), stream-ordered
void launch_write_surf_entries(hipStream_t s, SurfEntry* tab, int first, const SurfEntry* entries, int n);
// rows [r0, r1) of the n surfaces of entries[] (host memory) -> the same rows of n RGB frames of h x w: a conversion (YUV, raw Bayer), a
// permutation (BGR, RGBA, BGRA) -- k_rows_to_rgb<layout, true, ..> -- or a pitched copy (RGB: k_surf_copy_rows)
void launch_surf_rows_to_rgb(hipStream_t s, int layout, const SurfEntry* entries, YuvCoef k, uint8_t* rgb, size_t rgb_stride, int h, int w,
                             int r0, int r1, int n, const RawStages& raw = RawStages(), const RawSetEntry* rsets = nullptr,
                             const uint8_t* rids = nullptr);
// device sinks (k_sink.hip): n dense RGB frames of h x w, rgb_stride bytes apart -> the n surfaces of entries[] (host memory) in
// `layout`: a pitched copy (RGB) or a conversion with coeffs[8] (4:2:0; h and w even; sink_arith.h), 32 surfaces per launch
void launch_rgb_to_surfaces(hipStream_t s, int layout, const uint8_t* rgb, size_t rgb_stride, int h, int w, const SurfEntry* entries,
                            int n, const int32_t* coeffs);
// drawing into attached surfaces (k_inplace.hip).  The lane: the inverse-warp tables of the launch's calibration set and the row
// intervals of its first slot (span_stride_rows rows of (lo, hi) per slot); the text (nl == 0: none): glyph atlas, and the lines
// and character positions of the launch's first slot (slot_chars per slot); the rows: two disjoint runs [a0, a0 + an), [b0, b0 + bn).
struct InplaceLane {
    const int16_t* oxy;
    const uint16_t* ofrac;
    const int16_t* spans;
    size_t span_stride_rows;
    int bh, bw;
    float alpha;
};
struct InplaceText {
    const uint8_t *atlas, *advance, *lines;
    const int16_t* xpos;
    int first_char, n_glyphs, gw, gh, nl, len, slot_chars, y0, step;
};
struct InplaceRows { int a0, an, b0, bn; };
// the lane and the text of a launch whose first slot lies `at` slots behind the first slot of l and t
struct InplaceDraw { InplaceLane l; InplaceText t; };
inline InplaceDraw advanced(InplaceLane l, InplaceText t, int at) {
    l.spans += (size_t)at * l.span_stride_rows * 2;
    if (t.nl > 0) { t.lines += (size_t)at * t.slot_chars; t.xpos += (size_t)at * t.slot_chars; }
    return InplaceDraw{l, t};
}
// The inverse-warp tables of the calibration sets as the table-per-slot presentation kernels find them: entry `id` of the context's
// table of overlay tables (device memory, written when lt_overlay_configure_set builds a set's tables: with nothing in flight).  The
// sets of a launch's slots travel by value, as for the front end (CalIds).
struct OvTables {
    const int16_t* oxy;
    const uint16_t* ofrac;
};
static_assert(sizeof(OvTables) == 16, "OvTables: 16 bytes, one scalar load");
// Which tables a presentation launch over slots [first, first + n) uses: those of one set (sets == nullptr: the launcher's oxy /
// ofrac arguments, the kernels and arguments of a context with one set) or every slot's own -- ids[0, n), host memory, one launch
// per CalIds::N slots.
struct OvSets {
    const OvTables* sets = nullptr;
    const uint8_t* ids = nullptr;
};
// Lane and text into n surfaces in `layout`: tab[0, n) (device memory: the context's table from the launch's first slot), whose host
// mirror entries[0, n) decides the kernel (alignment).  rows4 = two runs of camera rows {a0, a1, b0, b1} outside which nothing can
// change (they may overlap or be empty).  kin / rgb2yuv[8]: 4:2:0 only.
// -> the launches enqueued
int launch_inplace(hipStream_t s, int layout, const SurfEntry* tab, const SurfEntry* entries, int n, int h, int w, const int rows4[4],
                   InplaceLane l, InplaceText t, YuvCoef kin, const int32_t* rgb2yuv, OvSets per_slot = OvSets());
// Lane and text drawn on the way from the slots' dense RGB camera frames into the caller's surfaces (k_draw_sink.hip): frame z of
// `rgb` (rgb_stride bytes apart) -> entries[z] (host memory) in `layout`, with the tables sets[ids[z]] and the row intervals and
// text of slot z from l.spans / t (l.oxy / l.ofrac are not read).  Lane lookups in camera rows [lane_r0, lane_r1) only, the glyph
// search in the text's rows only; every other row is a plain conversion.  SurfChunk::N surfaces per launch.  -> the launches enqueued
int launch_draw_to_surfaces(hipStream_t s, int layout, const uint8_t* rgb, size_t rgb_stride, int h, int w, const SurfEntry* entries,
                            int n, const OvTables* sets, const uint8_t* ids, InplaceLane l, InplaceText t, int lane_r0, int lane_r1,
                            const int32_t* coeffs);
void launch_split_bev(hipStream_t s, const uint8_t* bev, size_t bev_stride, int npix, const uint16_t* gamma_tab,
                      const uint16_t* cbrt_tab, const int32_t* coeffs, uint8_t* planeR, uint8_t* planeB,
                      size_t plane_stride, int n);
void launch_undistorted_to_rgb(hipStream_t s, const uint32_t* und, size_t und_px, int first_slot, int nrows, int w, uint8_t* out,
                               int n);

// one no-op launch per kernel translation unit: loads its code object (lt_create)
void preload_k_frontend(hipStream_t s);
void preload_k_filter(hipStream_t s);
void preload_k_tophat(hipStream_t s);
void preload_k_threshold(hipStream_t s);
void preload_k_threshold_walk(hipStream_t s);
void preload_k_threshold_mma(hipStream_t s);
void preload_k_adaptive_walk(hipStream_t s);
void preload_k_search(hipStream_t s);
void preload_k_overlay(hipStream_t s);

// presentation stage (k_overlay.hip)
// strip mode: only the camera rows [row0, row1) of every slot's annotated frame, packed, strip_stride bytes per slot; false: the
// geometry does not allow the four-pixel kernel (nothing launched)
bool launch_overlay_lane_strip(hipStream_t s, const uint8_t* frames, size_t frame_stride, uint8_t* strips, size_t strip_stride,
                               const int16_t* oxy, const uint16_t* ofrac, const int16_t* spans, size_t span_stride_rows, int img_w,
                               int row0, int row1, int bh, int bw, float alpha, int n);
// (-> the launches enqueued; per_slot: every slot with the tables of its own set, oxy / ofrac are not read then)
int launch_overlay_lane(hipStream_t s, const uint8_t* frames, uint8_t* out, size_t frame_stride, const int16_t* oxy,
                        const uint16_t* ofrac, const int16_t* spans, size_t span_stride_rows, int img_h, int img_w,
                        int bh, int bw, float alpha, int n, const int* rows4 = nullptr, OvSets per_slot = OvSets());
// one frame, the row intervals (host memory, bh pairs) passed as a kernel argument; rows4 = nullptr: the whole frame, else two
// runs of camera rows {a0, a1, b0, b1} (the others are not written); false: not launched (bh above LT_SPAN_ARG_ROWS, a row
// length that is no multiple of 4, or the runtime refused the argument block)
constexpr int LT_SPAN_ARG_ROWS = 1104;
void launch_store_word(hipStream_t s, unsigned* dev_word, unsigned value);
// (averaged coefficients at the start of every slot's interval region -> intervals: does that form exist for this height and these plot rows?)
bool lane_spans_from_regions_available(int bh, int n_rows);
bool launch_lane_spans_from_regions(hipStream_t s, const double* ploty, const double* ploty2, int n_rows, int bh, int bw, int16_t* spans, int n);
bool launch_lane_spans_from_fit(hipStream_t s, const lt_lane_record* rec, const double* prev_sum, int count, const double* ploty,
                                const double* ploty2, int n_rows, int bh, int bw, int16_t* spans);
bool launch_overlay_lane_one(hipStream_t s, const uint8_t* frame, uint8_t* out, const int16_t* oxy, const uint16_t* ofrac,
                             const int16_t* spans_host, int img_h, int img_w, int bh, int bw, float alpha, const int* rows4);
void launch_overlay_text(hipStream_t s, uint8_t* out, size_t frame_stride, int img_h, int img_w, const uint8_t* atlas,
                         const uint8_t* advance, int first_char, int n_glyphs, int gw, int gh, const uint8_t* lines,
                         const int16_t* xpos, int nl, int len, int slot_chars, int y0, int step, int n);   // slot_chars: characters between two slots' lines
// host -> device copy of a few hundred KB out of page-locked memory as a kernel launch (never blocks the caller)
void launch_copy_from_pinned(hipStream_t s, void* dst, const void* src_pinned, size_t bytes);
bool launch_copy_to_pinned(hipStream_t s, void* dst_pinned, const void* src, size_t bytes);   // false: not page-locked / aligned
bool launch_copy_rows_to_pinned(hipStream_t s, void* dst_pinned, const void* src, size_t pitch, size_t off, size_t bytes, int n);
bool launch_copy_words_to_pinned(hipStream_t s, void* dst_pinned, const void* src, size_t bytes);          // small, 4-byte granular
bool launch_mirror_record(hipStream_t s, void* dst_pinned, const void* src_record, unsigned ticket);       // a 64-byte record + the ticket word behind it
void launch_warp_rgb(hipStream_t s, const uint32_t* und, size_t und_px, int first_slot, const int16_t* wxy, const uint16_t* wfrac,
                     FrontEndGeom g, uint8_t* bev, size_t bev_stride, int n);

// dst = erode/dilate(src) with the ellipse; if minuend != nullptr: dst = sat(minuend - result)
void launch_morph_ellipse(hipStream_t s, const uint8_t* src, uint8_t* dst, const uint8_t* minuend, int h, int w,
                          const EllipseSE& se, bool dilate, size_t plane_stride, int n);
// decomposed 29x29 / 55x55 ellipses (k_tophat.hip); same contract as launch_morph_ellipse
// dpitch > 0: the destination has its own row pitch and per-frame stride (the padded top-hat planes the threshold walks read)
// copy_dst (55x55 top-hat with dpitch > 0 only): the minuend is stored there as well, in the destination's layout; false
// when that form is not available for the geometry (nothing was launched)
// zone: scratch of the split-band form (k_tophat.hip: k_morph_split), `stride_dwords` per frame of the launch; without one, or for
// a geometry tophat_split_form() refuses, the bands walk their halos (k_morph_runs2).  *form: 1 if the split-band form ran, else 0
struct MorphZone { uint32_t* base = nullptr; size_t stride_dwords = 0; };
// What a launcher call chose (lt_morph_planes, the test hook, hands it out): the kernel family, WIDE or narrow, the band cut, whether
// the last strip is a PAIR strip, the waves per task of k_morph_one / k_morph_one_pair (0 elsewhere).  launch_morph_one_pair cuts its
// two planes separately: nbands / band_rows are the 55x55 plane's, nbands29 / band_rows29 the 29x29 plane's (0 elsewhere).
enum { MORPH_NONE = 0, MORPH_ONE = 1, MORPH_ONE_PAIR = 2, MORPH_RUNS2 = 3, MORPH_SPLIT = 4, MORPH_ONE_ROW = 5 };
struct MorphReport { int family = MORPH_NONE, wide = 0, nbands = 0, band_rows = 0, pair_strip = 0, q = 0, nbands29 = 0, band_rows29 = 0; };
// force_bands > 0: that many bands instead of the launcher's own rule (what LT_MORPH_NB_* does in the experiments build; k_morph_one's
// bands stay even and at least 8 rows long)
bool launch_morph_runs(hipStream_t s, const uint8_t* src, uint8_t* dst, const uint8_t* minuend, int h, int w, int k,
                       bool dilate, size_t plane_stride, int n, int dpitch = 0, size_t dst_stride = 0, uint8_t* copy_dst = nullptr,
                       const MorphZone& zone = MorphZone(), int* form = nullptr, int force_bands = 0, MorphReport* report = nullptr);
// geometry -> form: true where the split-band form takes (h, w) cut into `nbands` bands of `band_rows` rows (the last one shorter)
bool tophat_split_form(int h, int w, int k, int band_rows, int nbands, bool wide);
int tophat_split_zone_rows(int k);          // rows of a boundary zone: 56 (55x55), 28 (29x29)
size_t tophat_split_zone_dwords(int k);     // scratch dwords per strip of a frame
// one or two frames: the same step of the 55x55 chain of one plane and of the 29x29 chain of another in one launch; false: not launched
bool launch_morph_one_pair(hipStream_t s, const uint8_t* src55, uint8_t* dst55, const uint8_t* min55, const uint8_t* src29, uint8_t* dst29,
                           const uint8_t* min29, int h, int w, bool dilate, size_t plane_stride, int n, int dpitch, size_t dst_stride,
                           int force_bands = 0, MorphReport* report = nullptr);
bool tophat_tables_match(const EllipseSE& se29, const EllipseSE& se55);
void launch_bilateral(hipStream_t s, const uint8_t* src, uint8_t* dst, int h, int w, int ksize, int C, int mode,
                      int tv, int fv, size_t plane_stride, int n);
void launch_adaptive_mean(hipStream_t s, const uint8_t* src, uint8_t* dst, int h, int w, int bs, int C,
                          size_t plane_stride, int n);
// the 'neighborhood' filter (lane_tracker.py:217-218) of both planes as running box sums (k_adaptive_walk.hip): out_r / out_b
// are the two thresholded bit planes.  false = outside its limits (nothing launched).
bool adaptive_walk_supported(int bs_r, int bs_b, int h, int w, size_t plane_stride);
bool launch_adaptive_walk(hipStream_t s, const uint8_t* R, int bs_r, int C_r, unsigned long long* out_r, const uint8_t* B, int bs_b,
                          int C_b, unsigned long long* out_b, int h, int w, size_t plane_stride, size_t bits_stride, int n);

// bit-plane path (k_threshold.hip): fused bilateral thresholds + merge, u8->bits merge, 5x5 open on bits
int launch_bilateral_bits(hipStream_t s, const uint8_t* thr, int k_r, int C_r, const uint8_t* thb, int k_b, int C_b,
                          const uint8_t* labb, int k_n, int C_n, int noise_thresh, int use_noise,
                          unsigned long long* bits, int h, int w, size_t plane_stride, size_t bits_stride, int n,
                          unsigned long long* bits_v = nullptr);   // bits_v: the V phases' verdicts as a partial plane of their own (two workgroups per tile)
void launch_pack_merge(hipStream_t s, const uint8_t* tr, const uint8_t* tb, const uint8_t* labb, const uint8_t* nb,
                       int noise_thresh, int use_noise, unsigned long long* bits, int h, int w, size_t plane_stride,
                       size_t bits_stride, int n);
void launch_open5_bits(hipStream_t s, const unsigned long long* merged, unsigned long long* eroded, uint8_t* mask, int h,
                       int w, size_t plane_stride, size_t bits_stride, int n);
// What the merged plane of the mask chain is on its way into the 5x5 open (host only):
//     (dst | more[0] | .. | more[n_more - 1]) & (and0 | and1)        -- the AND term only where the pair is given.
// dst already holds the first term, and the merged plane is written over it (lt_download_plane(4) reads it there).
struct MergeInputs {
    unsigned long long* dst = nullptr;
    const unsigned long long* more[3] = {nullptr, nullptr, nullptr};
    int n_more = 0;                                               // 0 (dst is the merged plane), 1 or 3
    const unsigned long long *and0 = nullptr, *and1 = nullptr;    // both or neither, and with n_more == 3 only (the greenery mask)
};
// the planes the kernels read for it -- their NP: 1, 2, 4 or 6 -- or 0 for a value that breaks the rules above (the one place they are checked)
inline int merge_planes(const MergeInputs& in) {
    if (!in.dst || (in.n_more != 0 && in.n_more != 1 && in.n_more != 3)) return 0;
    for (int i = 0; i < 3; ++i)
        if ((in.more[i] != nullptr) != (i < in.n_more)) return 0;
    if ((in.and0 != nullptr) != (in.and1 != nullptr) || (in.and0 && in.n_more != 3)) return 0;
    return in.and0 ? 6 : in.n_more + 1;
}
// both bilateral thresholds through the long-walk kernels (k_threshold_walk.hip): four partial bit planes, merged on the way into
// the open.  The top-hat planes have the row pitch `pitch` (a multiple of 64) and `plane_stride` bytes (a multiple of 64) per
// frame.  0 = ran, -1 = outside its limits: exactly where bilateral_walk_supported says no.
bool bilateral_walk_supported(int k_r, int C_r, int k_b, int C_b, int h, int w, int pitch, size_t plane_stride);
int launch_bilateral_walk(hipStream_t s, const uint8_t* thr, int k_r, int C_r, const uint8_t* thb, int k_b, int C_b,
                          unsigned long long* merged, unsigned long long* s1, unsigned long long* s2, unsigned long long* s3,
                          int h, int w, int pitch, size_t plane_stride, size_t bits_stride, int n);
// the same four partial planes, bit for bit, with the window sums as i8 matrix products (k_threshold_mma.hip), for the same calls:
// 0 = ran, -1 = bilateral_walk_supported says no, 1 = switched off (experiments build: LT_THRESHOLD_MMA=0), take the walks
int launch_bilateral_mma(hipStream_t s, const uint8_t* thr, int k_r, int C_r, const uint8_t* thb, int k_b, int C_b,
                         unsigned long long* merged, unsigned long long* s1, unsigned long long* s2, unsigned long long* s3,
                         int h, int w, int pitch, size_t plane_stride, size_t bits_stride, int n);
// the merge alone, in place (k_or4_bits); nothing to do for a plane that is merged already
void launch_or4_bits(hipStream_t s, const MergeInputs& in, int h, int w, size_t bits_stride, int n);
// the greenery mask (lane_tracker.py:223-225) through the walking kernels: noise_h | noise_v = !inRange(b, thresh, 255) |
// bilateral(b, 65, C_n); `braw` = the raw Lab-b plane with the padded pitch.  0 = ran, -1 = outside its limits.
bool noise_walk_supported(int k_n, int C_n, int h, int w, int pitch, size_t plane_stride);
int launch_noise_walk(hipStream_t s, const uint8_t* braw, int k_n, int C_n, int noise_thresh, unsigned long long* noise_h,
                      unsigned long long* noise_v, int h, int w, int pitch, size_t plane_stride, size_t bits_stride, int n);
// merge + erode + dilate with the 5x5 ellipse in one launch, bit planes in, bit plane out (k_merge_open5<NP>: a wave walks down
// the rows); false: not launched (a row wider than 64 words, a value merge_planes refuses, LT_OPEN5_SEPARATE=1)
bool launch_merge_open5(hipStream_t s, const MergeInputs& in, unsigned long long* opened, int h, int w, size_t bits_stride, int n);
// ... for a few frames: one launch of small workgroups (k_or_open5_small<NP>); false: as above, or LT_OPEN_SMALL=0
bool launch_or_open5_small(hipStream_t s, const MergeInputs& in, unsigned long long* opened, int h, int w, size_t bits_stride, int n);
// erode + dilate of a merged plane as two launches, bit plane out
void launch_open5_to_bits(hipStream_t s, const unsigned long long* merged, unsigned long long* eroded,
                          unsigned long long* opened, int h, int w, size_t bits_stride, int n);
void launch_bits_to_u8(hipStream_t s, const unsigned long long* bits, uint8_t* out, int h, int w, size_t plane_stride,
                       size_t bits_stride, int n);


struct SearchGeom {
    int h, w;                    // mask size
    int ww, wh, hw;              // window
    int img_height;              // h - ignore_bottom
    int img_center, y_start, nlevels, limit;
    int nbands;                  // column-sum bands per frame: max(nlevels, 1); band 0 = start slice
    int ignore_sides, search_range, def_left, def_right;
    int band_top, band_bottom;   // band search rows [top, bottom)
    double mu, bandwidth;
    int maxpix, maxlev;
};
// Per-frame block k_sws_fit2 leaves in the pixel buffer (u32 units): [0] nlev, [1] window height, [2] image
// height minus ignore_bottom, [3] 0; [4 ...) the (a, b) column range per (side, level); then, 8-byte aligned,
// one 64-bit column mask per (side, level, row): bit j = pixel (row, a + j) is set.
__host__ __device__ inline int sws2_mask_offset(int nlev) { return (4 + 4 * nlev + 1) & ~1; }
__host__ __device__ inline long long sws2_block_words(int nlev, int wh) { return sws2_mask_offset(nlev) + 4LL * nlev * wh; }
// k_band_fit2's per-frame block: [0] rows per side, [1] first row, [2..3] 0; int32 a per (side, row); then,
// 8-byte aligned, one u64 column mask per (side, row).  LDS: masks, a, width per row, 4 counters, 16 moments.
__host__ __device__ inline int band2_mask_offset(int nrows) { return (4 + 2 * nrows + 1) & ~1; }
__host__ __device__ inline long long band2_block_words(int nrows) { return band2_mask_offset(nrows) + 4LL * nrows; }
__host__ __device__ inline size_t band2_mom_offset(int nrows) { return ((size_t)2 * nrows * 16 + 16 + 15) & ~(size_t)15; }
// Mask input of the searches: u8 planes, or -- when `bits` is not null -- the opened bit plane the mask chain
// leaves (wpr words per row, bits_stride words per frame).  *_takes_bits tells whether the kernel version that
// would run for this geometry reads bit planes (the first-version kernels need u8 masks).
struct MaskBits {
    const unsigned long long* bits;
    size_t bits_stride;
    int wpr;
};
bool sws_fit_takes_bits(const SearchGeom& g, size_t mask_stride);
// false: the kernel this geometry selects needs more LDS than a workgroup can have (tall windows or bands wider than 64 columns
// on tall images, see k_search.hip) -- the entry points refuse the search with LT_ERR_INVALID
bool search_launchable(const SearchGeom& g, bool band, size_t mask_stride);
bool band_fit_takes_bits(const SearchGeom& g, size_t mask_stride);
void launch_sws_fit(hipStream_t s, const uint8_t* masks, size_t mask_stride, MaskBits mb, SearchGeom g, uint32_t* band_sums,
                    uint32_t* pix, int32_t* cent, lt_lane_record* rec, int n);
// previous coefficients of a single frame travel as a kernel argument (no upload, no synchronisation);
// batches read them from device memory
struct BandPrev {
    double c[6];
    int by_value;
};
void launch_band_fit(hipStream_t s, const uint8_t* masks, size_t mask_stride, MaskBits mb, SearchGeom g, const double* prev,
                     const BandPrev& bp, uint32_t* pix, lt_lane_record* rec, int n);

// the chained band search of one stream (k_band_chain2): slots [first, first + n) in order, frame k+1 around frame k's fit;
// the first frame around `seed` (by value) or, with seed.by_value == 0, around the fit in *seed_rec (device memory)
bool band_chain_supported(const SearchGeom& g, size_t mask_stride);
bool launch_band_fit_one(hipStream_t s, MaskBits mb, SearchGeom g, const BandPrev& bp, uint32_t* pix, lt_lane_record* rec,
                         size_t mask_stride, const int* zero, lt_lane_record* mirror, unsigned mirror_ticket);
void launch_band_chain(hipStream_t s, const uint8_t* masks, size_t mask_stride, MaskBits mb, SearchGeom g, const lt_lane_record* seed_rec,
                       const BandPrev& seed, uint32_t* pix, lt_lane_record* rec, int n, const int* cancel_epoch, int my_epoch);

// the searches of a list of (slot, mode, prev coefficients) items, one workgroup each (k_search_list), sliding-window items
// first (n_sws of them; their band sums by k_band_sums_bits over the same list).  Bit-plane masks only; supported: both kernels
// the list needs take bit planes for this geometry (null: no item of that mode).  `items` is device memory.
bool search_list_supported(const SearchGeom* gs, const SearchGeom* gb, size_t mask_stride);
void launch_search_list(hipStream_t s, const lt_search_item* items, int n, int n_sws, const uint8_t* masks, size_t mask_stride,
                        MaskBits mb, const SearchGeom& gs, const SearchGeom& gb, uint32_t* band_sums, uint32_t* pix, int32_t* cent,
                        lt_lane_record* rec);

// fit of one explicit pixel list (packed (y<<16)|x); out: 3 doubles + 1 flag double (1.0 = rank deficient)
void launch_fit_list(hipStream_t s, const uint32_t* pix, int n, int h, int w, double* out4);

// ---- search visualisation, cv2.resize(INTER_LINEAR) on u8 (k_search_viz.hip) ---------------------------------
// One picture of a k_search_viz launch: where the slot keeps what the picture is made of, and what the host adds.
struct VizFrame {
    const unsigned long long* bits;  // the slot's opened bit plane, or null: `mask`, its u8 plane (an uploaded mask)
    const uint8_t* mask;
    const uint32_t* pix;             // the slot's lane-pixel region, in the form rec->_pad names
    const int32_t* cent;             // the slot's window centroids [side][maxlev + 2] (kind 1)
    const lt_lane_record* rec;
    const int16_t* band;             // kind 2: [side][h] (lo, hi), the band polygons' row intervals clipped to the image (lo > hi: none)
    const int32_t* pts;              // (y, x) pairs of the new fit's plot points, left then right
    uint8_t* out;                    // h x w x 3
    int32_t kind, ww, wh, H1;        // lt_viz_item: kind, window_width, window_height, warp_h - ignore_bottom
    int32_t n_fit_left, n_fit_right;
};
constexpr int LT_VIZ_BATCH = 16;     // pictures per launch: their descriptors travel as a kernel argument
struct VizBatch {
    VizFrame f[LT_VIZ_BATCH];
};
// the first n pictures of the batch: the gather pass, then the lists (packed lane pixels, curves) on the same stream
void launch_search_viz(hipStream_t s, const VizBatch& b, int n, int h, int w, int wpr, int maxpix, int maxlev);
// n images of `ch` interleaved channels, rows of sw pixels, src_stride bytes apart -> columns [0, dcols) and all dh rows of the scaled
// images into columns dcol0 .. of destination rows of dpitch bytes; xt / yt: four int32 per destination column / row (tap 0, tap 1,
// coefficient 0, coefficient 1: utils._resize_taps), device memory
void launch_resize_linear_u8(hipStream_t s, const uint8_t* src, size_t src_stride, int sw, int ch, uint8_t* dst, size_t dst_stride,
                             int dpitch, int dcol0, int dcols, int dh, const int32_t* xt, const int32_t* yt, int n);
void preload_k_search_viz(hipStream_t s);

// ---- internal view of a context for lt_gather.cpp (defined in lt_api.cpp) ----------------------------
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // fills lt_last_error(), returns code
int ctx_device(lt_ctx* c);
int ctx_streams(lt_ctx* c, hipStream_t* out, int cap);        // the streams the slots currently run on; returns the count
int ctx_sync(lt_ctx* c);
int ctx_enqueue_records(lt_ctx* c, int first, int n, lt_lane_record* dst_device);
// every stream of the library comes from a per-process pool and goes back to it idle: none is ever destroyed (lt_api.cpp, StreamPool)
enum StreamKind { SK_COMPUTE = 0, SK_PLAIN, SK_CU_SET, SK_PRIORITY };
hipError_t stream_get(hipStream_t* st, StreamKind kind, int param);
void stream_put(hipStream_t st);

}  // namespace lt
