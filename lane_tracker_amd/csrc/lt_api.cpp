// C-ABI layer of liblane_tracker_amd.so (see include/lane_tracker_amd.h).
// Owns the context: HIP stream, calibration tables, frame slots; sequences the kernel chain of
// LaneTracker.find_lane_points() (lane_tracker.py:795-874) for a batch of independent frames (the mask stage: lt_mask_chain.cpp).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>
#include <immintrin.h>
#include <sys/mman.h>
#include <unistd.h>

#include <hip/hip_ext.h>

#include "front_arith.h"
#include "lt_ctx.h"
#include "resize_arith.h"

using namespace lt;

namespace {

thread_local std::string g_err;

}  // namespace

namespace lt {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char* kStageNames[LT_NUM_STAGES] = {"undistort_rows", "warp_split", "erode_r29", "tophat_r29", "erode_b55",
                                          "tophat_b55", "threshold", "merge", "open5", "sws_fit", "band_fit",
                                          "split_bev"};

int sync_all(lt_ctx* c) {
    for (int i = 0; i < c->nstreams && i < (int)c->streams.size(); ++i) HIP_TRY(hipStreamSynchronize(c->streams[i]));
    if (c->copy) HIP_TRY(hipStreamSynchronize(c->copy));
    if (c->search) HIP_TRY(hipStreamSynchronize(c->search));
    if (c->present) HIP_TRY(hipStreamSynchronize(c->present));
    if (c->urgent) HIP_TRY(hipStreamSynchronize(c->urgent));
    if (c->dl) HIP_TRY(hipStreamSynchronize(c->dl));
    c->spans_busy.lo = c->spans_busy.hi = 0;            // every overlay, every copy of the rest rows
    c->text_busy.lo = c->text_busy.hi = 0;
    c->annot_busy.lo = c->annot_busy.hi = 0;
    c->rest_pending = false;
    c->readers.reset();                                 // every reader / writer enqueued so far is done
    c->writers.reset();
    c->rests.reset();
    c->yuv_rows.reset();
    return LT_OK;
}

// work touching slots [lo, hi) has just been enqueued on `st`
int note_range(lt_ctx::RangeEvents& r, hipStream_t st, int lo, int hi) {
    unsigned cap = (unsigned)r.e.size();
    while (r.count > 0 && hipEventQuery(r.e[r.head].ev) == hipSuccess) {   // finished: nobody has to wait for it any more
        r.head = (r.head + 1) % cap;
        --r.count;
    }
    if (r.count == cap && cap < 4096) {        // everything in flight: a longer ring (the live entries first, in order)
        std::vector<lt_ctx::RangeEvents::Entry> bigger(2 * (size_t)cap, lt_ctx::RangeEvents::Entry{0, 0, nullptr});
        for (unsigned i = 0; i < r.count; ++i) bigger[i] = r.e[(r.head + i) % cap];
        r.e.swap(bigger);
        r.head = 0;
        cap *= 2;
    }
    if (r.count == cap) {
        r.overflow = true;
        r.head = (r.head + 1) % cap;
        --r.count;
    }
    lt_ctx::RangeEvents::Entry& w = r.e[(r.head + r.count) % cap];
    if (!w.ev && hipEventCreateWithFlags(&w.ev, hipEventDisableTiming) != hipSuccess) return fail(LT_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(w.ev, st));
    w.lo = lo;
    w.hi = hi;
    ++r.count;
    return LT_OK;
}
// One-frame calls of a context of one or two slots (LaneTracker.process(): capacity 2, one slot stream, the frame's kernels one
// behind the other on it): no event -- stream order is all the ordering the frame needs, and a hipEventRecord between two
// dependent kernels kept the second one waiting ~6 us (three of them on the way to the record: undistortion -> warp, open ->
// search, search -> lane spans).  Whoever waits from ANOTHER stream finds `lazy` set and waits for the slot stream's tail.
int note_range_frame(lt_ctx* c, lt_ctx::RangeEvents& r, hipStream_t st, int lo, int hi) {
    if (c->capacity <= 2 && !c->urgent_on && !c->stage_timing && c->nstreams == 1 && st == c->stream) {
        r.lazy = true;
        ++r.lazy_seq;
        return LT_OK;
    }
    return note_range(r, st, lo, hi);
}
// `waiter` waits for the entries that touch slots [lo, hi); *precise = false if the ring has overflowed or work was enqueued
// without an event (the caller then waits for stream tails)
int wait_range(const lt_ctx::RangeEvents& r, hipStream_t waiter, int lo, int hi, bool* precise) {
    *precise = !r.overflow && !r.lazy;
    if (r.overflow) return LT_OK;
    for (unsigned i = 0; i < r.count; ++i) {
        const lt_ctx::RangeEvents::Entry& w = r.e[(r.head + i) % (unsigned)r.e.size()];
        if (w.lo < hi && w.hi > lo) HIP_TRY(hipStreamWaitEvent(waiter, w.ev, 0));
    }
    return LT_OK;
}
int note_written(lt_ctx* c, hipStream_t st, int lo, int hi) { return note_range(c->writers, st, lo, hi); }
static int note_written_frame(lt_ctx* c, hipStream_t st, int lo, int hi, int n_call) {
    return n_call == 1 ? note_range_frame(c, c->writers, st, lo, hi) : note_range(c->writers, st, lo, hi);
}

// `st` waits for the chains still outstanding (not collected) that read or write slots [lo, hi): ticket by ticket, so that work on
// a frame in front of a running chain -- the second try of a failed frame while the frames behind it are already chained -- does
// not wait for that chain
int wait_chains(lt_ctx* c, hipStream_t st, int lo, int hi) {
    for (const auto& t : c->chains)
        if (t.first < hi && t.first + t.n > lo) HIP_TRY(hipStreamWaitEvent(st, t.done, 0));
    return LT_OK;
}

int flush_stage_events(lt_ctx* c) {
    if (c->pending.empty()) return LT_OK;
    { int rc = sync_all(c); if (rc) return rc; }
    for (auto& p : c->pending) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
        c->stage_ms[p.stage] += ms;
        c->stage_launches[p.stage] += 1;
    }
    c->pending.clear();
    c->ev_used = 0;
    return LT_OK;
}

int wait_tail(lt_ctx* c, hipStream_t waiter, hipStream_t st) {
    hipEvent_t e = next_order_event(c);
    if (!e) return fail(LT_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(e, st));
    HIP_TRY(hipStreamWaitEvent(waiter, e, 0));
    return LT_OK;
}

// Fallback of the stream-ordered uploads when the ring of readers has overflowed: `waiter` waits for the tail of every stream
// a kernel that reads camera frames can be on -- the slots' compute streams (undistortion), the presentation stream (overlays)
// and the urgent stream.
int wait_reader_tails(lt_ctx* c, hipStream_t waiter) {
    const bool slices_only = !c->readers.overflow;     // (only `lazy`: the unrecorded readers are on the slots' streams)
    auto tail = [&](hipStream_t st) { return !st || st == waiter ? (int)LT_OK : wait_tail(c, waiter, st); };
    for (int i = 0; i < c->nstreams && i < (int)c->streams.size(); ++i) { const int rc = tail(c->streams[i]); if (rc) return rc; }
    if (slices_only) return LT_OK;
    int rc = tail(c->present);
    if (!rc) rc = tail(c->urgent);
    return rc;
}
// A stream-ordered copy into the camera rows of slots [first, first + n) waits on `st` for the kernels that still read them (slot-range
// events), or -- where the ring does not know them all -- for the tails of every stream such a kernel can be on.
int wait_camera_readers(lt_ctx* c, hipStream_t st, int first, int n) {
    bool precise = true;
    int rc = wait_range(c->readers, st, first, first + n, &precise);
    if (!rc && !precise) rc = wait_reader_tails(c, st);
    return rc;
}

hipEvent_t next_order_event(lt_ctx* c) {
    constexpr size_t RING = 64;
    if (c->order_events.size() < RING) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        c->order_events.push_back(e);
        return e;
    }
    hipEvent_t e = c->order_events[c->order_next];
    c->order_next = (c->order_next + 1) % RING;
    return e;
}

int check_slots(lt_ctx* c, int first, int n) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (first < 0 || n < 0 || first + n > c->capacity)
        return fail(LT_ERR_CAPACITY, "slots [%d, %d) outside reserved capacity %d", first, first + n, c->capacity);
    return LT_OK;
}

int set_device(lt_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    return LT_OK;
}

void free_slots(lt_ctx* c) {
    dev_free(c->d_frames);
    dev_free(c->d_yuv);
    dev_free(c->d_src);
    dev_free(c->d_und);
    dev_free(c->d_surf);
    c->surf.clear();
    c->attached.clear();
    c->drawn.clear();
    dev_free(c->d_bev);
    c->masks.release();
    c->mask_bits_ok.clear();
    c->mask_u8_ok.clear();
    c->frame_full.clear();
    c->annot_full.clear();
    c->front_ok.clear();
    c->slot_cal.clear();
    c->slot_raw.clear();
    dev_free(c->d_rec);
    dev_free(c->d_prev);
    dev_free(c->d_pix);
    dev_free(c->d_cent);
    dev_free(c->d_band_sums);
    dev_free(c->d_spans);
    dev_free(c->d_ploty);
    c->h_ploty.clear();
    dev_free(c->d_annot);
    dev_free(c->d_strip);
    viz_free_device(c);
    c->maxbands = 0;
    c->capacity = 0;
    c->maxpix = 0;
    c->maxlev = 0;
    c->have_mask = false;
}

// Grow the per-slot result buffers.  Results of earlier searches stay readable (a tracker may fetch its lane
// pixels lazily, after a later search with other parameters enlarged the buffers): the old rows -- one per
// (slot, side) -- are copied to their new positions.
template <class T>
int grow_rows(lt_ctx* c, T** buf, size_t old_row, size_t new_row) {
    T* fresh = nullptr;
    int rc = dev_alloc(&fresh, (size_t)c->capacity * 2 * new_row);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(fresh, 0, (size_t)c->capacity * 2 * new_row * sizeof(T), c->stream));
    if (*buf && old_row)
        HIP_TRY(hipMemcpy2DAsync(fresh, new_row * sizeof(T), *buf, old_row * sizeof(T), old_row * sizeof(T),
                                 (size_t)c->capacity * 2, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    dev_free(*buf);
    *buf = fresh;
    return LT_OK;
}

int ensure_search_buffers(lt_ctx* c, int maxpix, int maxlev) {
    if (maxpix > c->maxpix) {
        { int rc = sync_all(c); if (rc) return rc; }
        int rc = grow_rows(c, &c->d_pix, (size_t)c->maxpix, (size_t)maxpix);
        if (rc) return rc;
        c->maxpix = maxpix;
    }
    if (maxlev > c->maxlev) {
        { int rc = sync_all(c); if (rc) return rc; }
        int rc = grow_rows(c, &c->d_cent, c->maxlev ? (size_t)c->maxlev + 2 : 0, (size_t)maxlev + 2);
        if (rc) return rc;
        c->maxlev = maxlev;
    }
    return LT_OK;
}

// Which slots hold their whole camera frame / whole annotated frame (see lt_ctx.h): the row-run entry points leave the other rows
// of a slot as whatever the block held before -- device memory comes back from the cache dirty -- and a whole-frame call on such
// a slot would hand out another stream's pixels.
void mark_frames(lt_ctx* c, int first, int n, int full) {
    for (int i = first; i < first + n && i < (int)c->frame_full.size(); ++i) c->frame_full[(size_t)i] = (uint8_t)full;
}
void front_stale(lt_ctx* c, int first, int n) {             // new camera rows in these slots: their planes are the old frames'
    for (int i = first; i < first + n && i < (int)c->front_ok.size(); ++i) c->front_ok[(size_t)i] = 0;
}
// an upload of camera rows into these slots: their front end reads the slots' own frames again (lt_attach_device_frames)
void detach_slots(lt_ctx* c, int first, int n) {
    for (int i = first; i < first + n && i < (int)c->attached.size(); ++i) c->attached[(size_t)i] = 0;
    for (int i = first; i < first + n && i < (int)c->drawn.size(); ++i) c->drawn[(size_t)i] = 0;
}
void mark_annot(lt_ctx* c, int first, int n, int full) {
    for (int i = first; i < first + n && i < (int)c->annot_full.size(); ++i) c->annot_full[(size_t)i] = (uint8_t)full;
}
int first_partial(const std::vector<uint8_t>& v, int first, int n) {
    for (int i = first; i < first + n && i < (int)v.size(); ++i)
        if (!v[(size_t)i]) return i;
    return -1;
}

int ensure_band_sums(lt_ctx* c, int nbands) {
    if (nbands <= c->maxbands) return LT_OK;
    int rc = sync_all(c);
    if (rc) return rc;
    dev_free(c->d_band_sums);
    if ((rc = dev_alloc(&c->d_band_sums, (size_t)c->capacity * nbands * c->calib.warp_w))) return rc;
    c->maxbands = nbands;
    return LT_OK;
}

// one no-op launch per kernel translation unit, once per process and device: their code objects load now (a few ms each), not under
// the first window of a stream or the first frame of a video
static void preload_kernels(int device, hipStream_t s) {
    static std::mutex m;
    static std::vector<int> done;
    std::lock_guard<std::mutex> g(m);
    if (std::find(done.begin(), done.end(), device) != done.end()) return;
    done.push_back(device);
    TraceScope ts_("lt_create:preload_kernels");
    preload_k_frontend(s);
    preload_k_filter(s);
    preload_k_tophat(s);
    preload_k_threshold(s);
    preload_k_threshold_walk(s);
    preload_k_threshold_mma(s);
    preload_k_adaptive_walk(s);
    preload_k_search(s);
    preload_k_overlay(s);
    preload_k_search_viz(s);
    (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
}

int ensure_bev(lt_ctx* c) {
    if (c->d_bev) return LT_OK;
    return dev_alloc(&c->d_bev, (size_t)c->capacity * c->bev_bytes);
}

void mark_masks(lt_ctx* c, int first, int n, int bits_ok, int u8_ok) {
    for (int i = first; i < first + n && i < (int)c->mask_bits_ok.size(); ++i) {
        c->mask_bits_ok[(size_t)i] = (uint8_t)bits_ok;
        c->mask_u8_ok[(size_t)i] = (uint8_t)u8_ok;
    }
}
bool masks_have_bits(const lt_ctx* c, int first, int n) {
    for (int i = first; i < first + n; ++i)
        if (!c->mask_bits_ok[(size_t)i]) return false;
    return true;
}
// the u8 mask plane of the slots; slots nobody has written a mask to read as zeros
static int ensure_mask_plane(lt_ctx* c) {
    if (c->masks.d_plane[P_MASK]) return LT_OK;
    const int rc = c->masks.ensure_plane(P_MASK);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->masks.d_plane[P_MASK], 0, (size_t)c->capacity * c->masks.plane_bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LT_OK;
}
// what the mask chain takes from the context besides the arena (lt_mask_chain.cpp)
static ChainEnv chain_env(lt_ctx* c) {
    return ChainEnv{&c->se29, &c->se55, c->brute_tophat, c->walk_min_pixels, &c->streams, c->stage_timing ? c : nullptr,
                    &c->last_threshold_path, &c->last_adaptive_path, &c->last_tophat_path, &c->last_threshold_form,
                    &c->last_open_form};
}
// make d_plane[P_MASK] current for the slots (expands the bit plane where only that exists)
int ensure_u8_masks(lt_ctx* c, int first, int n) {
    bool any = false;
    for (int i = first; i < first + n; ++i) any = any || !c->mask_u8_ok[(size_t)i];
    int rc = ensure_mask_plane(c);
    if (rc) return rc;
    if (!any) return LT_OK;
    if ((rc = sync_all(c))) return rc;
    for (int i = first; i < first + n;) {
        if (c->mask_u8_ok[(size_t)i]) { ++i; continue; }
        int j = i;
        while (j < first + n && !c->mask_u8_ok[(size_t)j]) ++j;
        launch_bits_to_u8(c->stream, slot_bits(c, i, true).bits, slot_mask(c, i),
                          c->calib.warp_h, c->calib.warp_w, c->masks.plane_bytes, c->masks.bits_stride, j - i);
        for (int k = i; k < j; ++k) c->mask_u8_ok[(size_t)k] = 1;
        i = j;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LT_OK;
}

int make_search_geom(lt_ctx* c, const lt_search_params* p, bool band, SearchGeom& g) {
    if (!p) return fail(LT_ERR_INVALID, "null search params");
    const int h = c->calib.warp_h, w = c->calib.warp_w;
    std::memset(&g, 0, sizeof g);
    g.h = h;
    g.w = w;
    if (p->ignore_bottom < 0 || p->ignore_bottom > h) return fail(LT_ERR_INVALID, "ignore_bottom out of range");
    if (!(p->partial >= 0.0 && p->partial <= 1.0)) return fail(LT_ERR_INVALID, "partial must be in [0,1]");
    g.img_height = h - p->ignore_bottom;                                      // lane_tracker.py:277
    if (band) {
        if (p->bandwidth < 0) return fail(LT_ERR_INVALID, "bandwidth must be >= 0");
        g.bandwidth = (double)p->bandwidth;
        g.band_bottom = h - p->ignore_bottom;                                 // :465
        g.band_top = (int)((double)h * (1.0 - p->partial));                   // :466 (2017 NumPy: int())
        if (g.band_top < 0) g.band_top = 0;
        const long long per_row = std::min<long long>(w, 2LL * p->bandwidth + 2);
        const int nrows = std::max(g.band_bottom - g.band_top, 0);
        long long need = (long long)nrows * per_row;
        g.maxpix = (int)std::min<long long>(std::max<long long>(need, 64), (long long)h * w);
        // (room for k_band_fit2's block whatever the bandwidth: which kernel runs must not depend on the searches before this one)
        g.maxpix = (int)std::max<long long>(g.maxpix, band2_block_words(nrows));
        g.maxlev = 1;
        return LT_OK;
    }
    if (p->window_width < 1 || p->window_height < 1) return fail(LT_ERR_INVALID, "window size must be >= 1");
    if (p->window_height > h) return fail(LT_ERR_INVALID, "window_height exceeds the image height");
    if (p->ignore_sides < 0 || p->search_range < 0) return fail(LT_ERR_INVALID, "negative margin/range");
    g.ww = p->window_width;
    g.wh = p->window_height;
    g.hw = (int)(p->window_width / 2.0);                                      // int(window_width/2)
    // A window whose first column is negative is an empty NumPy slice (:299, :319, :371, :409) -- as long as the image is at least as wide as the
    // window.  In a narrower image the negative start wraps round to columns of the right edge and the reference reports them with
    // negative x: nothing the kernels (or a caller) can hold, so such a search is refused.
    if (2 * g.hw > w) return fail(LT_ERR_INVALID, "window_width %d is wider than the image (%d columns)", p->window_width, w);
    g.img_center = (int)(w / 2.0);                                            // :278
    g.y_start = (int)((1.0 - p->start_slice) * g.img_height);                 // :279
    g.nlevels = (int)((p->partial * g.img_height) / p->window_height);        // :282
    if (g.nlevels < 0) g.nlevels = 0;
    g.limit = p->no_success_limit;
    g.ignore_sides = p->ignore_sides;
    g.search_range = p->search_range;
    g.def_left = (int)(w * 0.4);                                              // :308
    g.def_right = (int)(w * 0.6);                                             // :328
    g.mu = p->mu;
    const long long need = (long long)std::max(g.nlevels, 1) * g.wh * std::min(2 * g.hw, w);
    g.maxpix = (int)std::max<long long>(need, 64);
    // (room for k_sws_fit2's block however narrow the window: which kernel runs must not depend on the searches before this one)
    g.maxpix = (int)std::max<long long>(g.maxpix, sws2_block_words(std::max(g.nlevels, 1), g.wh));
    g.maxlev = std::max(g.nlevels, 1) + 1;
    g.nbands = std::max(g.nlevels, 1);
    return LT_OK;
}

// The set-up every search entry point shares: the geometry of `p`, search buffers large enough for it (and, for the sliding
// window, its band sums), and the buffers' actual row sizes in the geometry -- the kernels address slots by them.
int prepare_search(lt_ctx* c, const lt_search_params* p, bool band, SearchGeom& g) {
    int rc = make_search_geom(c, p, band, g);
    if (rc) return rc;
    if ((rc = ensure_search_buffers(c, g.maxpix, band ? 1 : g.maxlev))) return rc;
    if (!band && (rc = ensure_band_sums(c, g.nbands))) return rc;
    g.maxpix = c->maxpix;
    g.maxlev = c->maxlev;
    if (!search_launchable(g, band, c->masks.plane_bytes))
        return band ? fail(LT_ERR_INVALID, "a band search wider than 64 columns (bandwidth > 31), or any on an image taller than 8192 rows, "
                                           "keeps 16 bytes of LDS per image row: at most 9590 rows, this image has %d", g.h)
                    : fail(LT_ERR_INVALID, "this sliding-window search keeps 16 bytes of LDS per window row and 8 per image column: "
                                           "window_height %d is too tall for width %d (150 KB in all)", g.wh, g.w);
    return LT_OK;
}

// The searches read the opened bit plane of slots [first, first + n) when all of them have one and the kernel that will run for
// this geometry takes it (mode 0: sliding window, 1: band); else the u8 masks (ensure_u8_masks).
bool slot_reads_bits(const lt_ctx* c, const SearchGeom& g, int mode, int first, int n) {
    return masks_have_bits(c, first, n) && (mode == 0 ? sws_fit_takes_bits(g, c->masks.plane_bytes) : band_fit_takes_bits(g, c->masks.plane_bytes));
}

// The streams that carry the slot slices' kernels.  The HIP runtime multiplexes the streams of a process onto a
// small pool of hardware queues PER PRIORITY LEVEL (4 by default), in creation order -- so in a process that already
// holds other streams (torch's, RCCL's) two slices can land on one queue and stop overlapping (measured: 9 % of the
// batch rate under torch.distributed).  The slices therefore take the highest priority level, whose pool nothing
// else in the process uses; LT_STREAM_PRIORITY=normal restores plain streams.
// reserved > 0 (lt_set_search_cus): the stream is kept off CUs 0 .. reserved-1 (bits of the CU mask), which the search stream
// has to itself -- see lt_set_search_cus.  hipExtStreamCreateWithCUMask takes no priority, so a CU-masked stream has the
// runtime's default priority and LT_STREAM_PRIORITY has no effect on it: the priority only serves to put the slices of an
// independent-batch context on separate hardware queues (contexts that never call lt_set_search_cus), while a stream
// context runs its slices back to back behind the bus anyway.
static hipError_t make_compute_stream(hipStream_t* st, int reserved) {
    if (reserved > 0) {
        uint32_t mask[8];
        for (auto& w : mask) w = 0xffffffffu;
        for (int i = 0; i < reserved && i < 256; ++i) mask[i >> 5] &= ~(1u << (i & 31));
        return hipExtStreamCreateWithCUMask(st, 8, mask);
    }
    const char* e = LT_EXP_ENV("LT_STREAM_PRIORITY");
    int least = 0, greatest = 0;
    if ((e && strcmp(e, "normal") == 0) || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest)
        return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    return hipStreamCreateWithPriority(st, hipStreamNonBlocking, greatest);
}

// Streams are never destroyed: a context takes them from a per-process pool (by device, kind and CU reservation) and gives them
// back, idle, when it goes.  hipStreamDestroy can hang on this runtime: destroy one stream and, within a few milliseconds,
// another one that was created with hipExtStreamCreateWithCUMask -- the second call waits in AMDKFD_IOC_WAIT_EVENTS for good
// (tools/microbench/close_hang.hip: 9 of 9 runs; with 50 ms between the last work and the destroys, or the masked stream
// destroyed first, 0 of 8).  That was the close() of NOTES C.8 (round 4's library: 8 of 10 runs of tools/close_hang.py).  No
// ordering inside lt_destroy is safe against a second tracker's streams, so none is destroyed; a stream that has been idle in
// the pool is as good as a new one, and lt_create saves 20 ms per priority stream it no longer creates.
namespace {
struct StreamPool {
    struct Key { int device, kind, param; bool operator<(const Key& o) const { return std::tie(device, kind, param) < std::tie(o.device, o.kind, o.param); } };
    std::mutex m;
    std::map<Key, std::vector<hipStream_t>> idle;
    std::map<hipStream_t, Key> out;
};
StreamPool& stream_pool() { static StreamPool* p = new StreamPool; return *p; }
}  // namespace

hipError_t stream_get(hipStream_t* st, StreamKind kind, int param) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    StreamPool& sp = stream_pool();
    const StreamPool::Key key{dev, (int)kind, param};
    {
        std::lock_guard<std::mutex> g(sp.m);
        auto& v = sp.idle[key];
        if (!v.empty()) {
            *st = v.back();
            v.pop_back();
            sp.out[*st] = key;
            return hipSuccess;
        }
    }
    hipError_t e = hipSuccess;
    if (kind == SK_COMPUTE) e = make_compute_stream(st, param);
    else if (kind == SK_PLAIN) e = hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    else if (kind == SK_CU_SET) {        // the first `param` CUs and nothing else (the chained search), or -- param < 0 -- CUs 1 .. -param - 1 (the copy kernel)
        uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (param >= 0) for (int i = 0; i < param && i < 256; ++i) mask[i >> 5] |= 1u << (i & 31);
        else for (int b = 1; b < -param && b < 256; ++b) mask[b >> 5] |= 1u << (b & 31);
        e = hipExtStreamCreateWithCUMask(st, 8, mask);
    } else {                             // SK_PRIORITY: the highest priority level
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        e = hipStreamCreateWithPriority(st, hipStreamNonBlocking, hi);
    }
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> g(sp.m);
        sp.out[*st] = key;
    }
    return e;
}

void stream_put(hipStream_t st) {
    if (!st) return;
    (void)hipStreamSynchronize(st);
    StreamPool& sp = stream_pool();
    std::lock_guard<std::mutex> g(sp.m);
    auto it = sp.out.find(st);
    if (it == sp.out.end()) return;      // not ours: left alone
    sp.idle[it->second].push_back(st);
    sp.out.erase(it);
}

hipError_t create_compute_stream(hipStream_t* st, int reserved) { return stream_get(st, SK_COMPUTE, reserved); }

}  // namespace lt

// ================================================================================================
extern "C" {

const char* lt_last_error(void) { return g_err.c_str(); }
int lt_abi_version(void) { return LT_ABI_VERSION; }

int lt_device_count(int* count) {
    if (!count) return fail(LT_ERR_INVALID, "null count");
    HIP_TRY(hipGetDeviceCount(count));
    return LT_OK;
}

const char* lt_stage_name(int stage) { return stage >= 0 && stage < LT_NUM_STAGES ? kStageNames[stage] : ""; }

int lt_create(const lt_calib* calib, int device, lt_ctx** out) {
    if (!calib || !out) return fail(LT_ERR_INVALID, "null argument");
    if (calib->img_w < 2 || calib->img_h < 2 || calib->warp_w < 2 || calib->warp_h < 2 || calib->img_w > 16384 ||
        calib->img_h > 16384 || calib->warp_w > 4096 || calib->warp_h > 16384)
        return fail(LT_ERR_INVALID, "camera size must be in [2, 16384], bird's-eye width in [2, 4096], height in [2, 16384]");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(LT_ERR_HIP, "no HIP device visible: the lane-tracker kernels need a GPU (gfx950)");
    if (device < 0 || device >= ndev) return fail(LT_ERR_INVALID, "device %d out of range (%d visible)", device, ndev);
    TraceScope ts_all("lt_create");
    lt_ctx* c = new lt_ctx();
    c->calib = *calib;
    c->device = device;
    auto bail = [&](int rc) {
        lt_destroy(c);
        return rc;
    };
    if (const char* e = LT_EXP_ENV("LT_WALK_MIN_FRAMES")) c->walk_min_pixels = atoll(e) * calib->warp_w * calib->warp_h;   // (experiments build; the API: lt_set_walk_min_frames)
    if (hipSetDevice(device) != hipSuccess) return bail(fail(LT_ERR_HIP, "hipSetDevice(%d) failed", device));
    if (hipGetDeviceProperties(&c->prop, device) != hipSuccess) return bail(fail(LT_ERR_HIP, "hipGetDeviceProperties failed"));
    if (create_compute_stream(&c->stream) != hipSuccess) return bail(fail(LT_ERR_HIP, "hipStreamCreate failed"));
    c->streams.assign(1, c->stream);
    c->nstreams = 1;
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) return bail(fail(LT_ERR_HIP, "hipEventCreate failed"));
    if (stream_get(&c->copy, SK_PLAIN, 0) != hipSuccess) return bail(fail(LT_ERR_HIP, "copy stream creation failed"));

    // host tables
    const double t_tables = trace_on() ? trace_now() : 0.0;
    RemapTable warp, und;
    build_warp_table(*calib, warp);
    int r0 = 0, r1 = 0;
    warp_source_rows(*calib, warp, r0, r1);
    build_undistort_table(*calib, r0, r1, und);
    c->fe = FrontEndGeom{calib->img_h, calib->img_w, calib->warp_h, calib->warp_w, r0, r1 - r0};
    {
        int lo = calib->img_h, hi = 0;
        for (size_t o = 0; o < (size_t)und.rows * und.cols; ++o) {   // (the vectors carry one padding entry)
            const int sx = und.xy[o * 2], sy = und.xy[o * 2 + 1];
            if (sy < -1 || sy >= calib->img_h || sx < -1 || sx >= calib->img_w) continue;   // every tap outside: reads as 0
            lo = std::min(lo, std::max(sy, 0));
            hi = std::max(hi, std::min(sy + 2, calib->img_h));
        }
        c->cam_r0 = hi > lo ? lo : 0;
        c->cam_r1 = hi > lo ? hi : 0;
    }
    uint16_t gamma_tab[256], cbrt_tab[3072];
    int32_t coef[9];
    build_lab_tables(gamma_tab, cbrt_tab, coef);
    c->lab_clamp_dead = fa::lab_clamp_is_dead(*std::max_element(gamma_tab, gamma_tab + 256), coef);
    auto make_se = [](int k, EllipseSE& se) {
        int dx[64];
        ellipse_halfwidths(k, dx);
        se.k = k;
        for (int i = 0; i < 64; ++i) se.dx[i] = (int8_t)(i < k ? dx[i] : 0);
    };
    make_se(5, c->se5);
    make_se(29, c->se29);
    make_se(55, c->se55);
    if (!tophat_tables_match(c->se29, c->se55))
        return bail(fail(LT_ERR_STATE, "compiled-in ellipse run tables disagree with getStructuringElement's formula"));
    {
        const char* e = LT_EXP_ENV("LT_TOPHAT_BRUTE");
        c->brute_tophat = e && e[0] == '1';
    }

    if (trace_on()) trace_line("lt_create:host_tables", t_tables);
    TraceScope ts_up("lt_create:table_upload");
    int rc;
    if ((rc = dev_alloc(&c->d_wxy, warp.xy.size()))) return bail(rc);
    if ((rc = dev_alloc(&c->d_wfrac, warp.frac.size()))) return bail(rc);
    if ((rc = dev_alloc(&c->d_uxy, und.xy.size()))) return bail(rc);
    if ((rc = dev_alloc(&c->d_ufrac, und.frac.size()))) return bail(rc);
    if ((rc = dev_alloc(&c->d_gamma, 256))) return bail(rc);
    if ((rc = dev_alloc(&c->d_cbrt, 3072))) return bail(rc);
    if ((rc = dev_alloc(&c->d_coef, 9))) return bail(rc);
    hipError_t e = hipSuccess;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess && bytes) e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    };
    up(c->d_wxy, warp.xy.data(), warp.xy.size() * 2);
    up(c->d_wfrac, warp.frac.data(), warp.frac.size() * 2);
    up(c->d_uxy, und.xy.data(), und.xy.size() * 2);
    up(c->d_ufrac, und.frac.data(), und.frac.size() * 2);
    up(c->d_gamma, gamma_tab, sizeof gamma_tab);
    up(c->d_cbrt, cbrt_tab, sizeof cbrt_tab);
    up(c->d_coef, coef, sizeof coef);
    if (e != hipSuccess) return bail(fail(LT_ERR_HIP, "table upload failed: %s", hipGetErrorString(e)));

    preload_kernels(device, c->stream);
    c->frame_bytes = (size_t)calib->img_h * calib->img_w * 3;
    c->yuv_bytes = c->frame_bytes / 2;
    c->yuv_stride = (c->yuv_bytes + 15) & ~(size_t)15;
    c->und_bytes = (size_t)c->fe.nrows * calib->img_w * 3;   // as returned by lt_download_undistorted (RGB)
    c->und_px = (size_t)c->fe.nrows * calib->img_w;
    c->masks.set_geometry(calib->warp_h, calib->warp_w);
    c->bev_bytes = c->masks.plane_bytes * 3;
    c->cal.resize(1);                    // set 0: this calibration
    c->cal[0].calib = *calib;
    c->cal[0].r0 = r0;
    c->cal[0].r1 = r1;
    c->cal[0].need0 = c->cam_r0;
    c->cal[0].need1 = c->cam_r1;
    refresh_cal0(c);
    *out = c;
    return LT_OK;
}

void lt_destroy(lt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // Everything this context has in flight ends here, on EVERY stream it owns: its device memory goes back to the cache below
    // (dev_free), not through hipFree -- which used to wait for the whole device -- and the next context may be handed the very
    // same blocks at once (a cancelled chain still runs one more frame; copies may be queued on the download stream).
    static const bool trace = std::getenv("LT_TRACE_DESTROY") != nullptr;     // where a close() that does not return is waiting
    auto note = [&](const char* what) { if (trace) { std::fprintf(stderr, "lt_destroy: %s\n", what); std::fflush(stderr); } };
    note("streams of the slots");
    for (auto st : c->streams) if (st) (void)hipStreamSynchronize(st);
    {
        const char* names[5] = {"copy", "search", "present", "urgent", "dl"};
        hipStream_t sts[5] = {c->copy, c->search, c->present, c->urgent, c->dl};
        for (int i = 0; i < 5; ++i) if (sts[i]) { note(names[i]); (void)hipStreamSynchronize(sts[i]); }
    }
    // Streams, events and page-locked buffers go FIRST, device memory after them.  Round 4 released the memory first, and when the
    // cache then handed blocks back to the driver (hipFree of several GB), the hipStreamDestroy of the presentation stream -- a
    // stream with a CU mask -- that followed did not return: the thread sat in AMDKFD_IOC_WAIT_EVENTS for good (5 of 6 runs of
    // tools/close_hang.py with round 4's library; never once the stream is destroyed before the hipFree; NOTES D.5).
    // (LT_TRACE_DESTROY names every class of call.)
    note("events: timing pool, order ring, staging");
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    for (auto e : c->order_events) (void)hipEventDestroy(e);
    if (c->spans_busy.done) (void)hipEventDestroy(c->spans_busy.done);
    if (c->text_busy.done) (void)hipEventDestroy(c->text_busy.done);
    if (c->annot_busy.done) (void)hipEventDestroy(c->annot_busy.done);
    viz_free_host(c);
    note("streams back to the pool: dl");
    stream_put(c->dl);
    note("events: download timing");
    for (auto& d : c->dl_inflight) { (void)hipEventDestroy(d.a); (void)hipEventDestroy(d.b); }
    for (auto e : c->dl_event_pool) (void)hipEventDestroy(e);
    note("streams back to the pool: present, urgent");
    stream_put(c->present);
    stream_put(c->urgent);
    if (c->rest_done) (void)hipEventDestroy(c->rest_done);
    if (c->store_done) (void)hipEventDestroy(c->store_done);
    note("hipHostFree(spans, lines, xpos)");
    if (c->h_spans) (void)hipHostFree(c->h_spans);
    if (c->h_lines) (void)hipHostFree(c->h_lines);
    if (c->h_xpos) (void)hipHostFree(c->h_xpos);
    note("events: slot-range rings, chain tickets");
    for (auto& w : c->readers.e) if (w.ev) (void)hipEventDestroy(w.ev);
    for (auto& w : c->writers.e) if (w.ev) (void)hipEventDestroy(w.ev);
    for (auto& w : c->rests.e) if (w.ev) (void)hipEventDestroy(w.ev);
    for (auto& w : c->yuv_rows.e) if (w.ev) (void)hipEventDestroy(w.ev);
    for (auto& t : c->chains) (void)hipEventDestroy(t.done);
    for (auto e : c->chain_event_pool) (void)hipEventDestroy(e);
    note("hipHostFree(small, rec, rec_stage, cancel)");
    if (c->h_small) (void)hipHostFree(c->h_small);
    if (c->h_lists) (void)hipHostFree(c->h_lists);
    if (c->h_rec) (void)hipHostFree(c->h_rec);
    if (c->h_rec_stage) (void)hipHostFree(c->h_rec_stage);
    if (c->h_cancel) (void)hipHostFree(c->h_cancel);
    if (c->h_items) (void)hipHostFree(c->h_items);
    if (c->items_ev) (void)hipEventDestroy(c->items_ev);
    note("streams back to the pool: search, copy");
    stream_put(c->search);
    stream_put(c->copy);
    note("events: timer");
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    note("streams back to the pool: slot streams");
    for (auto st : c->streams) stream_put(st);
    if (c->streams.empty()) stream_put(c->stream);
    note("slots");
    FreeScope frees(c->device);          // one wait for the device instead of one per block; the blocks enter the cache together
    free_slots(c);
    note("tables and buffers");
    dev_free(c->d_uxy);
    dev_free(c->d_wxy);
    dev_free(c->d_ufrac);
    dev_free(c->d_wfrac);
    dev_free(c->d_gamma);
    dev_free(c->d_cbrt);
    dev_free(c->d_coef);
    dev_free(c->d_rs_xt);
    dev_free(c->d_rs_yt);
    raw_sets_release(c);
    raw_release(c->raw_dev);
    dev_free(c->d_stats);
    dev_free(c->d_oxy);
    dev_free(c->d_ofrac);
    for (size_t i = 1; i < c->cal.size(); ++i) {     // (set 0's tables are the ones above)
        lt_ctx::CalSet& q = c->cal[i];
        dev_free(q.d_uxy); dev_free(q.d_ufrac); dev_free(q.d_wxy); dev_free(q.d_wfrac); dev_free(q.d_oxy); dev_free(q.d_ofrac);
    }
    dev_free(c->d_cal);
    dev_free(c->d_ov);
    dev_free(c->d_atlas);
    dev_free(c->d_advance);
    dev_free(c->d_lines);
    dev_free(c->d_xpos);
    dev_free(c->d_items);
    note("done");
    delete c;
}

int lt_reserve(lt_ctx* c, int capacity) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (capacity < 1) return fail(LT_ERR_INVALID, "capacity must be >= 1");
    int rc = set_device(c);
    if (rc) return rc;
    if (capacity <= c->capacity) return LT_OK;
    TraceScope ts_all("lt_reserve", (size_t)capacity);
    if ((rc = sync_all(c))) return rc;
    // the old blocks are parked until the new ones are allocated and enter the device cache behind them (FreeScope, lt_memory.cpp):
    // the cache must not evict, to make room for the small blocks, the large ones this call is about to ask for
    FreeScope frees(c->device);
    {
        TraceScope ts_("lt_reserve:free_slots", (size_t)c->capacity);
        free_slots(c);
    }
    c->rec_mirror_slot = -1;
    c->capacity = capacity;
    const size_t n = (size_t)capacity;
    if ((rc = dev_alloc(&c->d_frames, n * c->frame_bytes + 16))) { free_slots(c); return rc; }   // +16: k_undistort_rows reads 8-byte windows
    c->direct_upload = -1;               // a new frame buffer: whether the host can write it is found out by the first small upload
    if (c->in_layout != LT_INPUT_RGB && (rc = dev_alloc(&c->d_yuv, n * c->yuv_stride + 16))) { free_slots(c); return rc; }
    if (c->src_w > 0 && (rc = dev_alloc(&c->d_src, n * c->src_stride))) { free_slots(c); return rc; }
    if ((rc = dev_alloc(&c->d_und, (size_t)((n + 1) / 2) * 2 * c->und_px))) { free_slots(c); return rc; }
    if ((rc = c->masks.reserve(capacity, true))) { free_slots(c); return rc; }
    c->mask_bits_ok.assign(n, 0);
    c->mask_u8_ok.assign(n, 1);          // zero-filled below
    c->frame_full.assign(n, 0);
    c->annot_full.assign(n, 0);
    c->front_ok.assign(n, 0);
    c->slot_cal.assign(n, 0);            // every slot starts with set 0
    c->slot_raw.assign(n, 0);            // ... and with raw set 0
    if ((rc = dev_alloc(&c->d_rec, n))) { free_slots(c); return rc; }
    if ((rc = dev_alloc(&c->d_prev, n * 6))) { free_slots(c); return rc; }
    c->capacity = capacity;
    TraceScope ts_ms("lt_reserve:memset");
    HIP_TRY(hipMemsetAsync(c->d_rec, 0, n * sizeof(lt_lane_record), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LT_OK;
}

// Everything a stream's first window (or a video's first frame) would otherwise set up on the way -- streams, page-locked
// staging, search buffers sized for these parameters, the presentation stage's buffers -- now, for the current capacity
// (lt_reserve first).  Nothing changes in what later calls compute; they find their buffers in place.
int lt_warm(lt_ctx* c, const lt_search_params* sws, const lt_search_params* band, int annotate) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (c->capacity < 1) return fail(LT_ERR_STATE, "lt_warm before lt_reserve");
    int rc = set_device(c);
    if (rc) return rc;
    TraceScope ts_all("lt_warm", (size_t)c->capacity);
    if ((rc = ensure_chain_buffers(c))) return rc;
    if (!c->urgent && create_compute_stream(&c->urgent, c->search_cus) != hipSuccess) return fail(LT_ERR_HIP, "hipStreamCreate failed");
    constexpr size_t SMALL = 256 << 10;
    if (!c->h_small && hipHostMalloc(reinterpret_cast<void**>(&c->h_small), SMALL, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        c->h_small = nullptr;
    }
    int maxpix = 0, maxlev = 0;
    if (sws) {
        SearchGeom g;
        if ((rc = make_search_geom(c, sws, false, g))) return rc;
        maxpix = std::max(maxpix, g.maxpix);
        maxlev = std::max(maxlev, g.maxlev);
        if ((rc = ensure_band_sums(c, g.nbands))) return rc;
    }
    if (band) {
        SearchGeom g;
        if ((rc = make_search_geom(c, band, true, g))) return rc;
        maxpix = std::max(maxpix, g.maxpix);
        maxlev = std::max(maxlev, 1);
    }
    if (maxpix && (rc = ensure_search_buffers(c, maxpix, maxlev))) return rc;
    // ... and the same refusal the run calls give (prepare_search), with the buffers as they now are
    SearchGeom g;
    if (sws && (rc = prepare_search(c, sws, false, g))) return rc;
    if (band && (rc = prepare_search(c, band, true, g))) return rc;
    if ((annotate & 3) && (rc = warm_presentation(c, (annotate & 3) == 2))) return rc;
    if ((annotate & 12) && (rc = warm_search_viz(c, (annotate & 8) != 0))) return rc;
    return sync_all(c);
}

int lt_get_info(lt_ctx* c, lt_info* out) {
    if (!c || !out) return fail(LT_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    out->abi_version = LT_ABI_VERSION;
    out->device = c->device;
    out->capacity = c->capacity;
    out->cu_count = c->prop.multiProcessorCount;
    out->src_row0 = c->fe.r0;
    out->src_row1 = c->fe.r0 + c->fe.nrows;
    out->max_pixels_per_side = c->maxpix;
    out->max_levels = c->maxlev;
    // compulsory input rows (full width, 3 B/px) + the mask written once
    out->alg_bytes_mask = (int64_t)c->fe.nrows * c->calib.img_w * 3 + (int64_t)c->masks.plane_bytes;
    out->alg_bytes_search = (int64_t)c->masks.plane_bytes + (int64_t)sizeof(lt_lane_record);
    std::snprintf(out->device_name, sizeof out->device_name, "%s", c->prop.name[0] ? c->prop.name : c->prop.gcnArchName);
    return LT_OK;
}

int lt_sync(lt_ctx* c) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    return sync_all(c);
}

int lt_set_streams(lt_ctx* c, int nstreams) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (nstreams < 1 || nstreams > 8) return fail(LT_ERR_INVALID, "nstreams must be in [1, 8]");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = sync_all(c))) return rc;
    if ((rc = flush_stage_events(c))) return rc;
    while ((int)c->streams.size() < nstreams) {
        hipStream_t st = nullptr;
        HIP_TRY(create_compute_stream(&st, c->search_cus));
        c->streams.push_back(st);
    }
    c->nstreams = nstreams;
    return LT_OK;
}

// ---- YUV input: 4:2:0 (NV12 / I420) and packed 4:2:2 (YUY2 / UYVY) ---------------------------------------
// OpenCV's 20-bit fixed-point conversion with the caller's five coefficients {CY, CVR, CVG, CUG, CUB}.  The kernels multiply with
// 24-bit instructions and add in int32: CY positive, every magnitude below 2^23, and no intermediate beyond int32.
static inline bool is_422(int layout) { return layout == LT_INPUT_YUY2 || layout == LT_INPUT_UYVY; }
static int check_yuv_format(int layout, const int32_t* k, int h, int w) {
    if (layout != LT_INPUT_NV12 && layout != LT_INPUT_I420 && !is_422(layout))
        return fail(LT_ERR_INVALID, "input layout must be RGB (0), NV12 (1), I420 (2), YUY2 (3), UYVY (4), BGR (5), RGBA (6), BGRA (7) or raw Bayer (16 .. 19; 10-bit 32 .. 35, 12-bit 48 .. 51)");
    if (!k) return fail(LT_ERR_INVALID, "a YUV layout needs its five conversion coefficients");
    if (is_422(layout)) {
        // (two macropixels a row at the least: the 8-byte window of a tap row lies inside its row)
        if (h < 1 || w < 4 || (w & 1)) return fail(LT_ERR_INVALID, "4:2:2 frames need an even width of at least 4, got %dx%d", w, h);
    } else if (h < 2 || w < 2 || (h & 1) || (w & 1)) return fail(LT_ERR_INVALID, "4:2:0 frames need an even width and height, got %dx%d", w, h);
    const long long lim = 1LL << 23;
    if (k[0] <= 0 || k[0] >= lim) return fail(LT_ERR_INVALID, "the luma coefficient must be in (0, 2^23)");
    for (int i = 1; i < 5; ++i)
        if (k[i] <= -lim || k[i] >= lim) return fail(LT_ERR_INVALID, "conversion coefficients must be below 2^23 in magnitude");
    const long long chroma = std::max({std::llabs((long long)k[1]), std::llabs((long long)k[2]) + std::llabs((long long)k[3]), std::llabs((long long)k[4])});
    if (239LL * k[0] + (1LL << 19) + 128LL * chroma > 0x7fffffffLL) return fail(LT_ERR_INVALID, "conversion coefficients overflow 32 bits");
    return LT_OK;
}

int lt_set_input_format(lt_ctx* c, int layout, const int32_t* coeffs) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    int rc;
    const bool plain = layout == LT_INPUT_RGB || is_rgb_family(layout) || is_raw_mosaic(layout);      // no coefficients: `coeffs` is not read
    if (is_raw_mosaic(layout)) {
        if ((rc = check_raw_size(layout, c->calib.img_h, c->calib.img_w))) return rc;
        // A packed row's bytes follow from the frame's width, so these layouts cannot name frames of another size at all: with an input size
        // they are a bad argument, as a layout number that does not exist is (the 16-bit layouts: LT_ERR_STATE, below)
        if (raw_packing(layout) >= 0 && c->src_w > 0)
            return fail(LT_ERR_INVALID, "MIPI-packed raw Bayer frames are not resized: a context with an input size (lt_set_input_size) takes RGB frames only");
    } else if (is_rgb_family(layout)) {
        // (the 8-byte window of a tap row starts at column min(x, W - 2): two pixels a row at the least)
        if (c->calib.img_w < 2) return fail(LT_ERR_INVALID, "BGR / RGBA / BGRA frames need a width of at least 2, got %dx%d", c->calib.img_w, c->calib.img_h);
    } else if (layout != LT_INPUT_RGB && (rc = check_yuv_format(layout, coeffs, c->calib.img_h, c->calib.img_w))) return rc;
    const bool same = layout == c->in_layout && (plain || std::memcmp(coeffs, c->yuv_coef, sizeof c->yuv_coef) == 0);
    if (same) return LT_OK;
    if (c->input_locked) return fail(LT_ERR_STATE, "the input format of a context cannot change after its first upload");
    if (layout != LT_INPUT_RGB && c->src_w > 0)
        return fail(LT_ERR_STATE, "a context with an input size (lt_set_input_size) takes RGB frames only: frames of another format are not resized");
    if ((rc = set_device(c))) return rc;
    if ((rc = sync_all(c))) return rc;
    if ((rc = raw_take_layout(c, layout))) return rc;  // (table, colour stage, shading map: before anything else of the context changes)
    if (layout == LT_INPUT_RGB) {
        dev_free(c->d_yuv);
    } else {
        // the staging frame of a slot: h w 3 / 2 bytes (4:2:0), h w 2 (4:2:2), h w 3 (BGR), h w 4 (RGBA / BGRA), h w (raw Bayer), 2 h w (10- /
        // 12-bit raw Bayer) or 5 h w / 4, 3 h w / 2 (the same MIPI-packed), slots a multiple of 16 apart
        const size_t row = (size_t)one_plane_row_bytes(layout, c->calib.img_w);
        const size_t bytes = row ? (size_t)c->calib.img_h * row : c->frame_bytes / 2, stride = (bytes + 15) & ~(size_t)15;
        if (stride != c->yuv_stride) dev_free(c->d_yuv);
        c->yuv_bytes = bytes;
        c->yuv_stride = stride;
        if (c->capacity > 0 && !c->d_yuv && (rc = dev_alloc(&c->d_yuv, (size_t)c->capacity * c->yuv_stride + 16))) {
            c->in_layout = LT_INPUT_RGB;     // (no staging: the context falls back to what needs none)
            (void)raw_take_layout(c, LT_INPUT_RGB);
            return rc;
        }
        if (!plain) std::memcpy(c->yuv_coef, coeffs, sizeof c->yuv_coef);
    }
    c->in_layout = layout;
    return LT_OK;
}

int lt_get_input_format(lt_ctx* c, int* layout, int32_t* coeffs) {
    if (!c || !layout) return fail(LT_ERR_INVALID, "null argument");
    *layout = c->in_layout;
    if (coeffs) std::memcpy(coeffs, c->yuv_coef, sizeof c->yuv_coef);
    return LT_OK;
}

// ---- input frames of another size (lt_set_input_size) ------------------------------------------------------------------------
// The slots' staging frames hold the caller's src_w x src_h RGB frames (or the rows of them that have been uploaded); k_resize_rows
// fills rows of the slots' RGB camera frames from them (lt_ingest.cpp: the resized kind).
int lt_set_input_size(lt_ctx* c, int src_w, int src_h) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (src_w < 1 || src_w > rz::SIZE_MAX_AXIS || src_h < 1 || src_h > rz::SIZE_MAX_AXIS)
        return fail(LT_ERR_INVALID, "an input size is 1 .. %d pixels wide and high, got %dx%d", rz::SIZE_MAX_AXIS, src_w, src_h);
    const int W = c->calib.img_w, H = c->calib.img_h;
    const bool plain = src_w == W && src_h == H;
    if (plain ? !resizes(c) : (src_w == c->src_w && src_h == c->src_h)) return LT_OK;
    if (c->input_locked) return fail(LT_ERR_STATE, "the input size of a context cannot change after its first upload");
    if (c->in_layout != LT_INPUT_RGB) return fail(LT_ERR_STATE, "an input size needs RGB frames: this context's input format is another layout");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = sync_all(c))) return rc;
    if (plain) {
        dev_free(c->d_src);
        dev_free(c->d_rs_xt);
        dev_free(c->d_rs_yt);
        c->rs_yt.clear();
        c->src_w = c->src_h = 0;
        c->src_bytes = c->src_stride = 0;
        return LT_OK;
    }
    // the tap tables: columns as the kernel reads them (padded to whole groups of four with entries that read column 0), rows as taps
    std::vector<uint32_t> xt((size_t)((W + 3) & ~3) * 2, 0u);
    for (int x = 0; x < W; ++x) rz::pack_column(rz::resize_tap(src_w, W, x), src_w, &xt[2 * (size_t)x]);
    std::vector<int32_t> yt((size_t)H * 4);
    for (int y = 0; y < H; ++y) {
        const rz::Tap t = rz::resize_tap(src_h, H, y);
        yt[4 * (size_t)y] = t.tap0; yt[4 * (size_t)y + 1] = t.tap1; yt[4 * (size_t)y + 2] = t.c0; yt[4 * (size_t)y + 3] = t.c1;
    }
    dev_free(c->d_rs_xt);
    dev_free(c->d_rs_yt);
    if ((rc = dev_alloc(&c->d_rs_xt, xt.size()))) return rc;
    if ((rc = dev_alloc(&c->d_rs_yt, yt.size()))) return rc;
    HIP_TRY(hipMemcpy(c->d_rs_xt, xt.data(), xt.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_rs_yt, yt.data(), yt.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    // the staging frame of a slot: src_h src_w 3 bytes, slots a multiple of 16 apart with at least 16 bytes between two frames
    const size_t bytes = (size_t)src_h * src_w * 3, stride = ((bytes + 15) & ~(size_t)15) + 16;
    if (stride != c->src_stride) dev_free(c->d_src);
    if (c->capacity > 0 && !c->d_src && (rc = dev_alloc(&c->d_src, (size_t)c->capacity * stride))) {
        dev_free(c->d_rs_xt);
        dev_free(c->d_rs_yt);
        c->rs_yt.clear();
        c->src_w = c->src_h = 0;             // (no staging: the context falls back to what needs none)
        c->src_bytes = c->src_stride = 0;
        return rc;
    }
    c->rs_yt.swap(yt);
    c->src_w = src_w;
    c->src_h = src_h;
    c->src_bytes = bytes;
    c->src_stride = stride;
    return LT_OK;
}

int lt_get_input_size(lt_ctx* c, int* src_w, int* src_h) {
    if (!c || !src_w || !src_h) return fail(LT_ERR_INVALID, "null argument");
    *src_w = resizes(c) ? c->src_w : c->calib.img_w;
    *src_h = resizes(c) ? c->src_h : c->calib.img_h;
    return LT_OK;
}

// ---- data movement (host frames into slots: lt_ingest.cpp) ----------------------------------------
int lt_get_source_rows(lt_ctx* c, int* row0, int* row1) {
    if (!c || !row0 || !row1) return fail(LT_ERR_INVALID, "null argument");
    *row0 = c->cam_r0;
    *row1 = c->cam_r1;
    return LT_OK;
}

// ---- frames that are already in device memory ------------------------------------------------------------------------------------
// Every plane of every surface is checked on the host before anything is launched: device memory of this context's device, its
// whole extent inside one allocation.  Blocks of lt_device_alloc are known to the library (no query); for anything else the
// runtime is asked -- per allocation once within a call, and never remembered beyond it (the caller may free it afterwards).
}  // extern "C"
namespace lt {
int check_plane(int device, const void* p, size_t extent, int k, int i, KnownRange& memo) {
    if (!p) return fail(LT_ERR_INVALID, "surface %d: plane %d is a null pointer", k, i);
    const uintptr_t a = (uintptr_t)p;
    const void* base = nullptr;
    size_t size = 0;
    int dev = 0;
    if (cached_block_find(p, &base, &size, &dev)) {
        if (dev != device) return fail(LT_ERR_INVALID, "surface %d: plane %d lies on device %d, not on device %d", k, i, dev, device);
        if (a + extent > (uintptr_t)base + size)
            return fail(LT_ERR_INVALID, "surface %d: plane %d runs past the end of its allocation (%zu bytes from the pointer, %zu left)", k, i, extent,
                        (size_t)((uintptr_t)base + size - a));
        return LT_OK;
    }
    if (memo.size && a >= memo.base && a + extent <= memo.base + memo.size) return LT_OK;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LT_ERR_INVALID, "surface %d: plane %d (%p) is not device memory of this process's HIP runtime (a host pointer, or memory of another runtime)", k, i, p);
    }
    if (at.type != hipMemoryTypeDevice) return fail(LT_ERR_INVALID, "surface %d: plane %d (%p) is not device memory", k, i, p);
    if (at.device != device) return fail(LT_ERR_INVALID, "surface %d: plane %d lies on device %d, not on device %d", k, i, at.device, device);
    hipDeviceptr_t rb = nullptr;
    size_t rs = 0;
    if (hipMemGetAddressRange(&rb, &rs, (hipDeviceptr_t)const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LT_ERR_INVALID, "surface %d: plane %d (%p): the runtime does not know its allocation", k, i, p);
    }
    if (a < (uintptr_t)rb || a + extent > (uintptr_t)rb + rs)
        return fail(LT_ERR_INVALID, "surface %d: plane %d runs past the end of its allocation (%zu bytes from the pointer, %zu left)", k, i, extent,
                    a >= (uintptr_t)rb && a < (uintptr_t)rb + rs ? (size_t)((uintptr_t)rb + rs - a) : (size_t)0);
    memo.base = (uintptr_t)rb;
    memo.size = rs;
    return LT_OK;
}
}  // namespace lt
extern "C" {
namespace {
int check_surfaces(lt_ctx* c, const lt_device_surface* s, int n, SurfEntry* out) {
    const int H = c->calib.img_h, W = c->calib.img_w, layout = c->in_layout;
    const int row = one_plane_row_bytes(layout, W) ? one_plane_row_bytes(layout, W) : W, crow = layout == LT_INPUT_NV12 ? W : W / 2;
    constexpr int PITCH_MAX = (1 << 23) - 1;             // the kernels multiply rows and pitches with 24-bit instructions
    KnownRange memo;
    for (int k = 0; k < n; ++k) {
        const lt_device_surface& f = s[k];
        if (f.pitch < row) return fail(LT_ERR_INVALID, "surface %d: pitch %d is below the row's %d bytes", k, (int)f.pitch, row);
        if (f.pitch > PITCH_MAX) return fail(LT_ERR_INVALID, "surface %d: pitch %d is too large", k, (int)f.pitch);
        if (is_bayer_wide(layout) && raw_packing(layout) < 0 && (((uintptr_t)f.plane[0] | (uintptr_t)f.pitch) & 1))      // 16-bit words: read as such by the row conversion
            return fail(LT_ERR_INVALID, "surface %d: a plane of 16-bit samples needs an even address and an even pitch, got %p and %d", k, f.plane[0], (int)f.pitch);
        const size_t ext = (size_t)f.pitch * (size_t)(H - 1) + (size_t)row;
        if (ext >= ((size_t)1 << 31) - 8) return fail(LT_ERR_INVALID, "surface %d: a plane of %zu bytes is too large", k, ext);
        int rc = check_plane(c->device, f.plane[0], ext, k, 0, memo);
        if (rc) return rc;
        out[k] = SurfEntry{{(uint64_t)(uintptr_t)f.plane[0], 0, 0}, f.pitch, 0};
        if (one_plane_row_bytes(layout, W)) continue;                // one plane; chroma_pitch is not read
        if (f.chroma_pitch < crow) return fail(LT_ERR_INVALID, "surface %d: chroma pitch %d is below the row's %d bytes", k, (int)f.chroma_pitch, crow);
        if (f.chroma_pitch > PITCH_MAX) return fail(LT_ERR_INVALID, "surface %d: chroma pitch %d is too large", k, (int)f.chroma_pitch);
        const size_t cext = (size_t)f.chroma_pitch * (size_t)(H / 2 - 1) + (size_t)crow;
        if (cext >= ((size_t)1 << 31) - 8) return fail(LT_ERR_INVALID, "surface %d: a plane of %zu bytes is too large", k, cext);
        for (int i = 1; i <= (layout == LT_INPUT_I420 ? 2 : 1); ++i) {
            if ((rc = check_plane(c->device, f.plane[i], cext, k, i, memo))) return rc;
            out[k].plane[i] = (uint64_t)(uintptr_t)f.plane[i];
        }
        out[k].cpitch = f.chroma_pitch;
    }
    return LT_OK;
}
}  // namespace

int lt_attach_device_frames(lt_ctx* c, const lt_device_surface* surfaces, int first, int n) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (!surfaces) return fail(LT_ERR_INVALID, "null surfaces");
    if (c->src_w > 0)
        return fail(LT_ERR_STATE, "a context with an input size (lt_set_input_size) takes host frames only: frames in device memory are not resized");
    if (n == 0) return LT_OK;
    if ((rc = set_device(c))) return rc;
    std::vector<SurfEntry> ent((size_t)n);
    if ((rc = check_surfaces(c, surfaces, n, ent.data()))) return rc;     // nothing has been launched or changed
    if (!c->d_surf) {
        if ((rc = dev_alloc(&c->d_surf, (size_t)c->capacity))) return rc;
        c->surf.assign((size_t)c->capacity, SurfEntry{});
        c->attached.assign((size_t)c->capacity, 0);
    }
    c->input_locked = true;
    mark_frames(c, first, n, 0);         // the slots' own camera frames are the previous occupants' until lt_device_frames_rest
    front_stale(c, first, n);
    for (int i = 0; i < n; ++i) {
        c->surf[(size_t)(first + i)] = ent[(size_t)i];
        c->attached[(size_t)(first + i)] = 1;
        if ((size_t)(first + i) < c->drawn.size()) c->drawn[(size_t)(first + i)] = 0;
    }
    // The entries go into the table on the slots' own streams: behind everything launched over these slots there (the front end
    // that reads their previous entries) and ahead of whatever is launched next -- and behind readers on other streams.
    return for_each_slice(c, first, n, [&](hipStream_t st, int f0, int m) {
        const int wrc = wait_camera_readers(c, st, f0, m);
        if (wrc) return wrc;
        launch_write_surf_entries(st, c->d_surf, f0, ent.data() + (f0 - first), m);
        HIP_TRY(hipGetLastError());
        return (int)LT_OK;
    });
}

int lt_upload_masks(lt_ctx* c, const uint8_t* masks, int first, int n) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (!masks) return fail(LT_ERR_INVALID, "null masks");
    if ((rc = set_device(c))) return rc;
    if ((rc = sync_all(c))) return rc;
    if ((rc = ensure_mask_plane(c))) return rc;
    HIP_TRY(hipMemcpyAsync(slot_mask(c, first), masks, (size_t)n * c->masks.plane_bytes,
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_mask = true;
    mark_masks(c, first, n, 0, 1);
    return LT_OK;
}

// The same masks as bit planes, in the layout of d_bits_open (slot_bits): the searches then take their bit-plane kernels, and the
// u8 mask is expanded from the plane when somebody asks for it (ensure_u8_masks).  Bits at columns >= w are cleared on the way:
// every reader of the plane may rely on zero tails, as behind the mask chain.
int lt_upload_mask_bits(lt_ctx* c, const uint64_t* bits, int first, int n) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (!bits) return fail(LT_ERR_INVALID, "null masks");
    if ((rc = set_device(c))) return rc;
    if ((rc = sync_all(c))) return rc;
    if (!c->masks.d_bits_open) return fail(LT_ERR_STATE, "the context holds no bit planes");
    if (n == 0) return LT_OK;
    const int h = c->calib.warp_h, w = c->calib.warp_w, wpr = (w + 63) / 64;
    const size_t words = (size_t)h * wpr, stride = c->masks.bits_stride;
    const uint64_t* src = bits;
    std::vector<uint64_t> stage;
    if (w & 63) {
        const uint64_t live = ((uint64_t)1 << (w & 63)) - 1;
        stage.assign(bits, bits + (size_t)n * words);
        for (size_t r = 0; r < (size_t)n * h; ++r) stage[r * wpr + (wpr - 1)] &= live;
        src = stage.data();
    }
    unsigned long long* dst = c->masks.d_bits_open + (size_t)first * stride;
    if (stride == words) {
        HIP_TRY(hipMemcpyAsync(dst, src, (size_t)n * words * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    } else {
        for (int i = 0; i < n; ++i)
            HIP_TRY(hipMemcpyAsync(dst + (size_t)i * stride, src + (size_t)i * words, words * sizeof(unsigned long long),
                                   hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_mask = true;
    mark_masks(c, first, n, 1, 0);
    return LT_OK;
}

int lt_upload_bev(lt_ctx* c, const uint8_t* bev, int first, int n) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (!bev) return fail(LT_ERR_INVALID, "null image");
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_bev(c))) return rc;
    if ((rc = sync_all(c))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_bev + (size_t)first * c->bev_bytes, bev, (size_t)n * c->bev_bytes,
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LT_OK;
}

}  // extern "C"
namespace lt {
int download(lt_ctx* c, const void* src, void* dst, size_t bytes) {
    if (!dst) return fail(LT_ERR_INVALID, "null output buffer");
    int rc = set_device(c);
    if (rc) return rc;
    hipStream_t st = c->stream;
    if (c->urgent_on && c->urgent) st = c->urgent;      // lt_set_urgent: what is asked for was produced on the urgent stream (or is complete)
    else if ((rc = sync_all(c))) return rc;             // results may come from any of the context's streams
    // Records, headers, lane-pixel blocks: through a page-locked scratch buffer by a kernel launch, not the copy engine (23 us
    // for 64 bytes; behind the annotated frames of a stream, milliseconds).
    constexpr size_t SMALL = 256 << 10;
    if (bytes <= SMALL) {
        if (!c->h_small && hipHostMalloc(reinterpret_cast<void**>(&c->h_small), SMALL, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            c->h_small = nullptr;
        }
        if (c->h_small && launch_copy_words_to_pinned(st, c->h_small, src, bytes)) {
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(st));
            std::memcpy(dst, c->h_small, bytes);
            return LT_OK;
        }
    }
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LT_OK;
}
}  // namespace lt
extern "C" {

int lt_download_masks(lt_ctx* c, int first, int n, uint8_t* masks) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_u8_masks(c, first, n))) return rc;
    return download(c, slot_mask(c, first), masks, (size_t)n * c->masks.plane_bytes);
}

int lt_download_plane(lt_ctx* c, int plane, int first, int n, uint8_t* out) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    static const int map[6] = {P_R, P_B, P_THR, P_THB, P_MERGED, P_MASK};
    if (plane < 0 || plane > 5) return fail(LT_ERR_INVALID, "unknown plane %d", plane);
    if (plane == LT_PLANE_MASK) {
        if ((rc = set_device(c))) return rc;
        if ((rc = ensure_u8_masks(c, first, n))) return rc;
    }
    if (plane == LT_PLANE_MERGED) {   // kept bit-packed on the device; expand on demand
        if ((rc = set_device(c))) return rc;
        if ((rc = sync_all(c))) return rc;
        if ((rc = c->masks.ensure_plane(P_MERGED))) return rc;
        launch_bits_to_u8(c->stream, c->masks.d_bits_merged + (size_t)first * c->masks.bits_stride,
                          c->masks.d_plane[P_MERGED] + (size_t)first * c->masks.plane_bytes, c->calib.warp_h, c->calib.warp_w,
                          c->masks.plane_bytes, c->masks.bits_stride, n);
    }
    if (plane == LT_PLANE_TOPHAT_R || plane == LT_PLANE_TOPHAT_B) {   // slot by slot: the current copy may be the padded one
        if (!out) return fail(LT_ERR_INVALID, "null output buffer");
        if ((rc = set_device(c))) return rc;
        if ((rc = sync_all(c))) return rc;
        const int w = c->calib.warp_w, h = c->calib.warp_h, q = plane == LT_PLANE_TOPHAT_R ? 0 : 1;
        for (int i = first; i < first + n; ++i) {
            uint8_t* dst = out + (size_t)(i - first) * c->masks.plane_bytes;
            if (i < (int)c->masks.th_padded.size() && c->masks.th_padded[(size_t)i])
                HIP_TRY(hipMemcpy2DAsync(dst, (size_t)w, c->masks.d_th_pad[q] + (size_t)i * c->masks.th_pad_bytes, (size_t)c->masks.th_pitch, (size_t)w,
                                         (size_t)h, hipMemcpyDeviceToHost, c->stream));
            else
                HIP_TRY(hipMemcpyAsync(dst, c->masks.d_plane[map[plane]] + (size_t)i * c->masks.plane_bytes, c->masks.plane_bytes,
                                       hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        return LT_OK;
    }
    return download(c, c->masks.d_plane[map[plane]] + (size_t)first * c->masks.plane_bytes, out, (size_t)n * c->masks.plane_bytes);
}

int lt_download_undistorted(lt_ctx* c, int first, int n, uint8_t* out) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (!out) return fail(LT_ERR_INVALID, "null output buffer");
    if (n == 0 || c->und_bytes == 0) return LT_OK;
    if ((rc = set_device(c))) return rc;
    uint8_t* tmp = nullptr;
    if ((rc = sync_all(c))) return rc;
    if ((rc = dev_alloc(&tmp, (size_t)n * c->und_bytes))) return rc;
    launch_undistorted_to_rgb(c->stream, c->d_und, c->und_px, first, c->fe.nrows, c->fe.img_w, tmp, n);
    rc = download(c, tmp, out, (size_t)n * c->und_bytes);
    dev_free(tmp);
    return rc;
}

// ---- host-only views of the calibration tables lt_create builds (no GPU needed) --------------------------------
int lt_calib_source_rows(const lt_calib* calib, int* row0, int* row1) {
    if (!calib || !row0 || !row1) return fail(LT_ERR_INVALID, "null argument");
    RemapTable warp;
    build_warp_table(*calib, warp);
    warp_source_rows(*calib, warp, *row0, *row1);
    return LT_OK;
}

int lt_calib_warp_table(const lt_calib* calib, int16_t* xy, uint16_t* frac) {
    if (!calib || !xy || !frac) return fail(LT_ERR_INVALID, "null argument");
    RemapTable t;
    build_warp_table(*calib, t);
    const size_t n = (size_t)t.rows * t.cols;
    std::memcpy(xy, t.xy.data(), n * 2 * sizeof(int16_t));
    std::memcpy(frac, t.frac.data(), n * sizeof(uint16_t));
    return LT_OK;
}

int lt_calib_undistort_table(const lt_calib* calib, int row0, int row1, int16_t* xy, uint16_t* frac) {
    if (!calib || !xy || !frac) return fail(LT_ERR_INVALID, "null argument");
    if (row0 < 0 || row1 < row0 || row1 > calib->img_h) return fail(LT_ERR_INVALID, "rows [%d, %d) outside the image", row0, row1);
    RemapTable t;
    build_undistort_table(*calib, row0, row1, t);
    const size_t n = (size_t)t.rows * t.cols;
    std::memcpy(xy, t.xy.data(), n * 2 * sizeof(int16_t));
    std::memcpy(frac, t.frac.data(), n * sizeof(uint16_t));
    return LT_OK;
}

int lt_calib_lab_tables(uint16_t* gamma256, uint16_t* cbrt3072, int32_t* coeffs9) {
    if (!gamma256 || !cbrt3072 || !coeffs9) return fail(LT_ERR_INVALID, "null argument");
    build_lab_tables(gamma256, cbrt3072, coeffs9);
    return LT_OK;
}

int lt_calib_ellipse(int k, int32_t* halfwidths, int* taps) {
    if (k < 1 || k > 63 || !(k & 1) || !halfwidths || !taps) return fail(LT_ERR_INVALID, "k must be odd, 1..63");
    int dx[64];
    *taps = ellipse_halfwidths(k, dx);
    for (int i = 0; i < k; ++i) halfwidths[i] = dx[i];
    return LT_OK;
}

// A search over ONE slot (process(): one frame per call, the host waiting for its record) sends the record to page-locked
// memory by a launch queued right behind the search kernel, while the device is still busy with the frame: lt_download_records
// then waits for that stream and reads 64 bytes, instead of launching the copy once the search is over (8 us of 0.4 ms).
static lt_lane_record* rec_mirror_device(lt_ctx* c) {      // the mirror as kernels address it (nullptr: there is none)
    if (!c->h_rec && hipHostMalloc(reinterpret_cast<void**>(&c->h_rec), 256, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        c->h_rec = nullptr;
    } else if (c->h_rec && !c->rec_ticket_counter) {
        std::memset(c->h_rec, 0, 256);       // (the ticket word behind the record: no stale match)
        c->rec_ticket_counter = 1;
    }
    void* dev = nullptr;
    if (!c->h_rec || hipHostGetDevicePointer(&dev, c->h_rec, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return static_cast<lt_lane_record*>(dev);
}
static void mirror_record(lt_ctx* c, hipStream_t st, int slot) {
    c->rec_mirror_slot = -1;
    c->rec_ticket = 0;
    static_assert(sizeof(lt_lane_record) == 64, "k_mirror_record copies 16 words and stores the ticket behind them");
    unsigned ticket = ++c->rec_ticket_counter;
    if (!ticket) ticket = ++c->rec_ticket_counter;          // 0 means "no ticket"
    if (rec_mirror_device(c) && launch_mirror_record(st, c->h_rec, slot_rec(c, slot), ticket)) {
        c->rec_mirror_slot = slot;
        c->rec_mirror_stream = st;
        c->rec_ticket = ticket;
    }
}

int lt_download_records(lt_ctx* c, int first, int n, lt_lane_record* out) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (n == 1 && out && c->rec_mirror_slot == first && c->h_rec) {
        if ((rc = set_device(c))) return rc;
        // The search kernel stores its ticket behind the record: poll for it (hipStreamSynchronize returns 15-20 us after the
        // kernel's last store, the word is there within 2: tools/microbench/sync_latency.hip).  LT_RECORD_POLL=0: wait for the
        // stream (A/B); after 2 ms without the ticket likewise (an error would show there).
        static const bool poll = [] { const char* e = LT_EXP_ENV("LT_RECORD_POLL"); return !(e && e[0] == '0'); }();
        bool seen = false;
        if (poll && c->rec_ticket) {
            const volatile unsigned* word = reinterpret_cast<const volatile unsigned*>(c->h_rec + 1);
            const auto t0 = std::chrono::steady_clock::now();
            for (unsigned spins = 0; !(seen = *word == c->rec_ticket); ++spins) {
                __builtin_ia32_pause();
                if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
            }
            std::atomic_thread_fence(std::memory_order_acquire);
        }
        if (!seen) HIP_TRY(hipStreamSynchronize(c->rec_mirror_stream));
        std::memcpy(out, c->h_rec, sizeof(lt_lane_record));
        return LT_OK;
    }
    return download(c, slot_rec(c, first), out, (size_t)n * sizeof(lt_lane_record));
}

// The lane pixels of one side of a slot, expanded from the form the search kernels leave on the device (`region`: a host copy of the
// slot's list region, at least the words the record's format uses) into the reference's (y, x) lists, in the reference's order.
static int expand_pixels(const lt_ctx* c, const lt_lane_record& r, const uint32_t* region, size_t region_words, int side, int32_t* ys,
                         int32_t* xs, int cap, int* count) {
    if (r._pad == 1) {
        // k_sws_fit2 leaves one column mask per window row (lt_internal.h: sws2_mask_offset); the lists
        // self.left_y / left_x (level-major, row-major inside a window, ascending x) are expanded here
        const int nlev = (int)region[0], wh = (int)region[1], H1 = (int)region[2];
        const long long words = sws2_block_words(nlev, wh);
        if (nlev < 1 || wh < 1 || words > (long long)region_words) return fail(LT_ERR_STATE, "corrupt lane-pixel block");
        const int32_t* roi = reinterpret_cast<const int32_t*>(region + 4);
        const uint32_t* masks = region + sws2_mask_offset(nlev);
        int n = 0;
        for (int level = 0; level < nlev; ++level) {
            const int sl = side * nlev + level, a = roi[sl * 2], b = roi[sl * 2 + 1];
            if (b <= a) continue;
            for (int ry = 0; ry < wh; ++ry) {
                const size_t mi = ((size_t)sl * wh + ry) * 2;
                unsigned long long m = (unsigned long long)masks[mi] | ((unsigned long long)masks[mi + 1] << 32);
                const int y = H1 - (1 + level) * wh + ry;
                while (m) {
                    const int j = __builtin_ctzll(m);
                    m &= m - 1;
                    if (n < cap && ys && xs) { ys[n] = y; xs[n] = a + j; }
                    ++n;
                }
            }
        }
        *count = n;
        if (n > 0 && cap > 0 && (!ys || !xs)) return fail(LT_ERR_INVALID, "null pixel buffers");
        return LT_OK;
    }
    if (r._pad == 2) {
        // k_band_fit2: one column mask and one first column per (side, row); row-major, ascending x
        const int nrows = (int)region[0], top = (int)region[1];
        const long long words = band2_block_words(nrows);
        if (nrows < 0 || words > (long long)region_words) return fail(LT_ERR_STATE, "corrupt lane-pixel block");
        const int32_t* row_a = reinterpret_cast<const int32_t*>(region + 4) + (size_t)side * nrows;
        const uint32_t* masks = region + band2_mask_offset(nrows) + (size_t)side * nrows * 2;
        int n = 0;
        for (int ry = 0; ry < nrows; ++ry) {
            unsigned long long m = (unsigned long long)masks[2 * ry] | ((unsigned long long)masks[2 * ry + 1] << 32);
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                if (n < cap && ys && xs) { ys[n] = top + ry; xs[n] = row_a[ry] + j; }
                ++n;
            }
        }
        *count = n;
        if (n > 0 && cap > 0 && (!ys || !xs)) return fail(LT_ERR_INVALID, "null pixel buffers");
        return LT_OK;
    }
    // first-version kernels: packed (y << 16 | x) lists, side by side
    int n = side == 0 ? r.n_left : r.n_right;
    if (n > c->maxpix) n = c->maxpix;
    *count = n;
    if (n > cap) n = cap;
    if (n <= 0) return LT_OK;
    if (!ys || !xs) return fail(LT_ERR_INVALID, "null pixel buffers");
    const uint32_t* tmp = region + (size_t)side * c->maxpix;
    for (int i = 0; i < n; ++i) {
        ys[i] = (int32_t)(tmp[i] >> 16);
        xs[i] = (int32_t)(tmp[i] & 0xffffu);
    }
    return LT_OK;
}

int lt_download_pixels(lt_ctx* c, int slot, int side, int32_t* ys, int32_t* xs, int cap, int* count) {
    int rc = check_slots(c, slot, 1);
    if (rc) return rc;
    if (side < 0 || side > 1 || !count || cap < 0) return fail(LT_ERR_INVALID, "bad side/count/cap");
    if (!c->d_pix) return fail(LT_ERR_STATE, "no search has run yet");
    lt_lane_record r;
    if ((rc = download(c, slot_rec(c, slot), &r, sizeof r))) return rc;
    const uint32_t* block = slot_pix(c, slot);
    size_t words = 0;
    if (r._pad == 1 || r._pad == 2) {
        uint32_t hdr[4];
        if ((rc = download(c, block, hdr, sizeof hdr))) return rc;
        const long long w = r._pad == 1 ? sws2_block_words((int)hdr[0], (int)hdr[1]) : band2_block_words((int)hdr[0]);
        if (w < 4 || w > 2LL * c->maxpix) return fail(LT_ERR_STATE, "corrupt lane-pixel block");
        words = (size_t)w;
    } else {
        words = (size_t)c->maxpix + (size_t)std::min(std::max((int)r.n_right, 0), c->maxpix);     // both sides' lists, the right one as far as it goes
        if (side == 0) words = (size_t)std::min(std::max((int)r.n_left, 0), c->maxpix);
    }
    std::vector<uint32_t> blk(std::max<size_t>(words, 4));
    if (words && (rc = download(c, block, blk.data(), words * 4))) return rc;
    return expand_pixels(c, r, blk.data(), blk.size(), side, ys, xs, cap, count);
}

// Both sides' lane pixels and (want_centroids) both window-centroid lists of a slot in ONE round trip to the device: the record, the
// slot's list region and its centroid lists are copied into page-locked memory by three launches behind each other, the host waits
// once and expands.  LaneTracker fetches the lists of a search lazily -- when somebody reads lt.left_x, or when the NEXT search over
// the same slot is about to overwrite them (the second try of a frame, lane_tracker.py:1101: the first try's lists stay the
// tracker's if the second finds nothing) -- and did so through lt_download_pixels / lt_download_centroids: fourteen round trips,
// 300 us of a two-try frame (profiles/r06_config1_timeline.txt).  counts[2] / cent_counts[2] return the full lengths; lists longer
// than cap / cent_cap are cut (call again with larger buffers).  LT_ERR_CAPACITY: the slot's region does not fit the staging
// buffer (huge search windows) -- use lt_download_pixels / lt_download_centroids.
int lt_download_lane_lists(lt_ctx* c, int slot, int32_t* ly, int32_t* lx, int32_t* ry, int32_t* rx, int cap, int* counts, int want_centroids,
                           int32_t* cent_l, int32_t* cent_r, int cent_cap, int* cent_counts) {
    int rc = check_slots(c, slot, 1);
    if (rc) return rc;
    if (!counts || cap < 0 || (want_centroids && (!cent_counts || cent_cap < 0))) return fail(LT_ERR_INVALID, "lt_download_lane_lists: bad arguments");
    if (!c->d_pix) return fail(LT_ERR_STATE, "no search has run yet");
    if (want_centroids && !c->d_cent) return fail(LT_ERR_STATE, "no sliding-window search has run yet");
    if ((rc = set_device(c))) return rc;
    const size_t region_words = 2 * (size_t)c->maxpix, cent_words = want_centroids ? 2 * ((size_t)c->maxlev + 2) : 0;
    const size_t bytes = sizeof(lt_lane_record) + (region_words + cent_words) * 4;
    if (bytes > ((size_t)2 << 20)) return fail(LT_ERR_CAPACITY, "lt_download_lane_lists: the slot's list region (%zu bytes) exceeds the staging buffer", bytes);
    if (c->h_lists_bytes < bytes) {
        if (c->h_lists) (void)hipHostFree(c->h_lists);
        c->h_lists = nullptr;
        c->h_lists_bytes = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&c->h_lists), bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            c->h_lists = nullptr;
            return fail(LT_ERR_NOMEM, "hipHostMalloc(%zu) failed", bytes);
        }
        c->h_lists_bytes = bytes;
    }
    hipStream_t st = c->stream;
    if (c->urgent_on && c->urgent) st = c->urgent;      // as in download(): what is asked for was produced on the urgent stream (or is complete)
    else if ((rc = sync_all(c))) return rc;
    uint8_t* h = c->h_lists;
    bool ok = launch_copy_words_to_pinned(st, h, slot_rec(c, slot), sizeof(lt_lane_record)) &&
              launch_copy_words_to_pinned(st, h + sizeof(lt_lane_record), slot_pix(c, slot), region_words * 4);
    if (ok && cent_words) ok = launch_copy_words_to_pinned(st, h + sizeof(lt_lane_record) + region_words * 4, slot_cent(c, slot), cent_words * 4);
    if (!ok) return fail(LT_ERR_HIP, "lt_download_lane_lists: the copy launches were refused");
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    lt_lane_record r;
    std::memcpy(&r, h, sizeof r);
    const uint32_t* region = reinterpret_cast<const uint32_t*>(h + sizeof(lt_lane_record));
    if ((rc = expand_pixels(c, r, region, region_words, 0, ly, lx, cap, &counts[0]))) return rc;
    if ((rc = expand_pixels(c, r, region, region_words, 1, ry, rx, cap, &counts[1]))) return rc;
    if (want_centroids) {
        const int32_t* cw = reinterpret_cast<const int32_t*>(region + region_words);
        for (int side = 0; side < 2; ++side) {
            const int32_t* t = cw + (size_t)side * (c->maxlev + 2);
            int n = t[0];
            if (n < 0) n = 0;
            if (n > c->maxlev + 1) n = c->maxlev + 1;
            cent_counts[side] = n;
            int32_t* out = side == 0 ? cent_l : cent_r;
            for (int i = 0; i < n && i < cent_cap && out; ++i) out[i] = t[1 + i];
        }
    }
    return LT_OK;
}

int lt_download_centroids(lt_ctx* c, int slot, int side, int32_t* out, int cap, int* count) {
    int rc = check_slots(c, slot, 1);
    if (rc) return rc;
    if (side < 0 || side > 1 || !count || cap < 0 || (cap > 0 && !out)) return fail(LT_ERR_INVALID, "bad side/count/cap/out");
    if (!c->d_cent) return fail(LT_ERR_STATE, "no sliding-window search has run yet");
    std::vector<int32_t> tmp((size_t)c->maxlev + 2);
    if ((rc = download(c, slot_cent(c, slot) + (size_t)side * (c->maxlev + 2), tmp.data(), tmp.size() * 4))) return rc;
    int n = tmp[0];
    if (n < 0) n = 0;
    if (n > c->maxlev + 1) n = c->maxlev + 1;
    *count = n;
    for (int i = 0; i < n && i < cap; ++i) out[i] = tmp[1 + i];
    return LT_OK;
}

int lt_copy_records_to_device(lt_ctx* c, int first, int n, void* dst) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (!dst) return fail(LT_ERR_INVALID, "null destination");
    if ((rc = set_device(c))) return rc;
    if ((rc = sync_all(c))) return rc;
    HIP_TRY(hipMemcpyAsync(dst, slot_rec(c, first), (size_t)n * sizeof(lt_lane_record), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LT_OK;
}

int lt_enqueue_records_to_device(lt_ctx* c, int first, int n, void* dst) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (!dst) return fail(LT_ERR_INVALID, "null destination");
    if ((rc = set_device(c))) return rc;
    // stream-ordered behind the searches of each slot slice; no host synchronisation
    rc = for_each_slice(c, first, n, [&](hipStream_t st, int f0, int m) {
        HIP_TRY(hipMemcpyAsync(static_cast<lt_lane_record*>(dst) + (f0 - first), slot_rec(c, f0), (size_t)m * sizeof(lt_lane_record),
                               hipMemcpyDeviceToDevice, st));
        return (int)LT_OK;
    });
    return rc;
}

int lt_set_frame_base(lt_ctx* c, int first, int n, int first_frame) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    c->rec_mirror_slot = -1;                  // the records change: the page-locked mirror of a one-frame search is stale
    if ((rc = set_device(c))) return rc;
    std::vector<lt_lane_record> tmp((size_t)n);
    if (n == 0) return LT_OK;
    if ((rc = download(c, slot_rec(c, first), tmp.data(), tmp.size() * sizeof(lt_lane_record)))) return rc;
    for (int i = 0; i < n; ++i) tmp[i].frame = first_frame + i;
    HIP_TRY(hipMemcpyAsync(slot_rec(c, first), tmp.data(), tmp.size() * sizeof(lt_lane_record), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LT_OK;
}

// ---- calibration sets -----------------------------------------------------------------------------------
}  // extern "C"
namespace lt {
void refresh_cal0(lt_ctx* c) {
    if (c->cal.empty()) return;
    lt_ctx::CalSet& q = c->cal[0];
    q.d_uxy = c->d_uxy; q.d_ufrac = c->d_ufrac; q.d_wxy = c->d_wxy; q.d_wfrac = c->d_wfrac; q.d_oxy = c->d_oxy; q.d_ofrac = c->d_ofrac;
    q.have_overlay = c->have_overlay;
}
int refuse_foreign(lt_ctx* c, int first, int n, const char* who) {
    const int bad = first_foreign(c, first, n);
    if (bad < 0) return LT_OK;
    return fail(LT_ERR_STATE, "%s knows the context's own calibration only: slot %d has calibration set %d", who, bad, slot_set(c, bad));
}
// The rows every set shares, from what each set needs: the rows of the undistorted image (fe.r0, fe.nrows), the camera rows the
// uploads bring (cam_r0, cam_r1: widened by the lane's rows where those are the same run, as lt_overlay_configure says, and never
// narrowed) and the rows a lane can reach (ov_r0, ov_r1).  Returns whether the rows of the undistorted image changed.
bool union_rows(lt_ctx* c) {
    auto join = [](int& lo, int& hi, int a, int b) {
        if (b <= a) return;
        if (hi <= lo) { lo = a; hi = b; }
        else { lo = std::min(lo, a); hi = std::max(hi, b); }
    };
    int r0 = 0, r1 = 0, n0 = 0, n1 = 0, o0 = 0, o1 = 0;
    for (const auto& q : c->cal) {
        join(r0, r1, q.r0, q.r1);
        join(n0, n1, q.need0, q.need1);
        if (q.have_overlay) join(o0, o1, q.ov_r0, q.ov_r1);
    }
    if (n1 > n0 && o1 > o0 && o0 >= n0 - 32 && o1 <= n1 + 32) { n0 = std::min(n0, o0); n1 = std::max(n1, o1); }
    join(n0, n1, c->cam_r0, c->cam_r1);   // the rows the uploads bring only ever widen (a second lt_overlay_configure: as it always did)
    c->cam_r0 = n0; c->cam_r1 = n1;
    c->ov_r0 = o0; c->ov_r1 = o1;
    const bool changed = r0 != c->fe.r0 || r1 - r0 != c->fe.nrows;
    c->fe.r0 = r0;
    c->fe.nrows = r1 - r0;
    return changed;
}
// The undistortion table of calibration `k` for the rows [U0, U1) of the undistorted image, built and uploaded into fresh device
// blocks; need0 / need1: the camera rows it reads for the rows [r0, r1) the set's own warp reads.  Nothing of the context changes.
struct UndTables {
    int16_t* d_uxy = nullptr;
    uint16_t* d_ufrac = nullptr;
    int need0 = 0, need1 = 0;
    void release() { dev_free(d_uxy); dev_free(d_ufrac); }
};
static int build_undistortion(const lt_calib& k, int r0, int r1, int U0, int U1, UndTables& out) {
    RemapTable und;
    build_undistort_table(k, U0, U1, und);
    int lo = k.img_h, hi = 0;
    for (int row = std::max(r0, U0); row < std::min(r1, U1); ++row)
        for (int x = 0; x < und.cols; ++x) {
            const size_t o = (size_t)(row - U0) * und.cols + x;
            const int sx = und.xy[o * 2], sy = und.xy[o * 2 + 1];
            if (sy < -1 || sy >= k.img_h || sx < -1 || sx >= k.img_w) continue;   // every tap outside: reads as 0
            lo = std::min(lo, std::max(sy, 0));
            hi = std::max(hi, std::min(sy + 2, k.img_h));
        }
    out.need0 = hi > lo ? lo : 0;
    out.need1 = hi > lo ? hi : 0;
    int rc;
    if ((rc = dev_alloc(&out.d_uxy, und.xy.size())) || (rc = dev_alloc(&out.d_ufrac, und.frac.size()))) { out.release(); return rc; }
    if (hipMemcpy(out.d_uxy, und.xy.data(), und.xy.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(out.d_ufrac, und.frac.data(), und.frac.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        out.release();
        return fail(LT_ERR_HIP, "table upload failed");
    }
    return LT_OK;
}
// The set table for a context that has one calibration set only: the set-per-slot raw forms take the calibration's table per slot too.
int ensure_cal_table(lt_ctx* c) {
    if (c->d_cal) return LT_OK;
    int rc = dev_alloc(&c->d_cal, (size_t)LT_MAX_CALIBRATIONS);
    if (rc) return rc;
    refresh_cal0(c);
    const lt_ctx::CalSet& q = c->cal[0];
    const CalTables t{q.d_uxy, q.d_ufrac, q.d_wxy, q.d_wfrac};
    if (hipMemcpy(c->d_cal, &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess) {
        dev_free(c->d_cal);
        return fail(LT_ERR_HIP, "table upload failed: %s", hipGetErrorString(hipGetLastError()));
    }
    return LT_OK;
}

}  // namespace lt
extern "C" {

// Everything that can fail -- the new set's tables, the other sets' tables where the rows grow, the buffer of undistorted rows, the
// set table -- is built beside the context first; only then is the set committed, by steps that cannot fail.  An error leaves the
// context exactly as it was.
int lt_add_calibration(lt_ctx* c, const lt_calib* calib, int* id) {
    if (!c || !calib || !id) return fail(LT_ERR_INVALID, "null argument");
    if (calib->img_w != c->calib.img_w || calib->img_h != c->calib.img_h || calib->warp_w != c->calib.warp_w || calib->warp_h != c->calib.warp_h)
        return fail(LT_ERR_INVALID, "a calibration set must have the context's sizes (camera %dx%d, bird's-eye %dx%d), got %dx%d and %dx%d",
                    c->calib.img_w, c->calib.img_h, c->calib.warp_w, c->calib.warp_h, calib->img_w, calib->img_h, calib->warp_w, calib->warp_h);
    if (c->input_locked) return fail(LT_ERR_STATE, "calibration sets are added before a context's first upload");
    if ((int)c->cal.size() >= LT_MAX_CALIBRATIONS) return fail(LT_ERR_CAPACITY, "a context holds at most %d calibration sets", LT_MAX_CALIBRATIONS);
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = sync_all(c))) return rc;
    TraceScope ts_all("lt_add_calibration");
    refresh_cal0(c);
    lt_ctx::CalSet q;
    q.calib = *calib;
    RemapTable warp;
    build_warp_table(*calib, warp);
    warp_source_rows(*calib, warp, q.r0, q.r1);
    // the rows of the undistorted image with this set: do they grow?
    int U0 = c->fe.r0, U1 = c->fe.r0 + c->fe.nrows;
    if (q.r1 > q.r0) {
        if (U1 <= U0) { U0 = q.r0; U1 = q.r1; }
        else { U0 = std::min(U0, q.r0); U1 = std::max(U1, q.r1); }
    }
    const bool grow = U0 != c->fe.r0 || U1 - U0 != c->fe.nrows;
    const size_t n_old = c->cal.size(), und_px = (size_t)(U1 - U0) * c->calib.img_w;
    std::vector<UndTables> fresh(grow ? n_old + 1 : 1);      // [i]: set i's table for the new rows (grow), last: the new set's
    uint32_t* d_und = nullptr;
    CalTables* d_cal = nullptr;
    auto drop = [&](int code) {
        dev_free(q.d_wxy); dev_free(q.d_wfrac);
        for (auto& f : fresh) f.release();
        dev_free(d_und);
        dev_free(d_cal);
        return code;
    };
    if ((rc = dev_alloc(&q.d_wxy, warp.xy.size()))) return drop(rc);
    if ((rc = dev_alloc(&q.d_wfrac, warp.frac.size()))) return drop(rc);
    if (hipMemcpy(q.d_wxy, warp.xy.data(), warp.xy.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(q.d_wfrac, warp.frac.data(), warp.frac.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        return drop(fail(LT_ERR_HIP, "table upload failed"));
    }
    if (grow)        // every earlier set's table again, for the union
        for (size_t i = 0; i < n_old; ++i)
            if ((rc = build_undistortion(c->cal[i].calib, c->cal[i].r0, c->cal[i].r1, U0, U1, fresh[i]))) return drop(rc);
    if ((rc = build_undistortion(q.calib, q.r0, q.r1, U0, U1, fresh.back()))) return drop(rc);
    if (grow && c->capacity > 0 && (rc = dev_alloc(&d_und, (size_t)((c->capacity + 1) / 2) * 2 * und_px))) return drop(rc);
    if (!c->d_cal && (rc = dev_alloc(&d_cal, (size_t)LT_MAX_CALIBRATIONS))) return drop(rc);
    {   // the set table as it will be
        std::vector<CalTables> tabs(n_old + 1);
        for (size_t i = 0; i < n_old; ++i)
            tabs[i] = CalTables{grow ? fresh[i].d_uxy : c->cal[i].d_uxy, grow ? fresh[i].d_ufrac : c->cal[i].d_ufrac, c->cal[i].d_wxy, c->cal[i].d_wfrac};
        tabs[n_old] = CalTables{fresh.back().d_uxy, fresh.back().d_ufrac, q.d_wxy, q.d_wfrac};
        if (hipMemcpy(c->d_cal ? c->d_cal : d_cal, tabs.data(), tabs.size() * sizeof(CalTables), hipMemcpyHostToDevice) != hipSuccess) {
            // (an existing table may now name tables that are about to be dropped: written again below)
            (void)hipGetLastError();
            if (c->d_cal) {
                for (size_t i = 0; i < n_old; ++i) tabs[i] = CalTables{c->cal[i].d_uxy, c->cal[i].d_ufrac, c->cal[i].d_wxy, c->cal[i].d_wfrac};
                (void)hipMemcpy(c->d_cal, tabs.data(), n_old * sizeof(CalTables), hipMemcpyHostToDevice);
                (void)hipGetLastError();
            }
            return drop(fail(LT_ERR_HIP, "table upload failed"));
        }
    }
    // ---- commit: nothing below can fail ----
    if (d_cal) c->d_cal = d_cal;
    if (grow) {
        for (size_t i = 0; i < n_old; ++i) {
            lt_ctx::CalSet& e = c->cal[i];
            dev_free(e.d_uxy);
            dev_free(e.d_ufrac);
            e.d_uxy = fresh[i].d_uxy;
            e.d_ufrac = fresh[i].d_ufrac;
            e.need0 = fresh[i].need0;
            e.need1 = fresh[i].need1;
        }
        c->d_uxy = c->cal[0].d_uxy;          // (set 0's tables are the context's own)
        c->d_ufrac = c->cal[0].d_ufrac;
        c->und_px = und_px;
        c->und_bytes = und_px * 3;           // as returned by lt_download_undistorted (RGB)
        if (c->capacity > 0) {
            dev_free(c->d_und);
            c->d_und = d_und;
        }
        std::fill(c->front_ok.begin(), c->front_ok.end(), 0);
    }
    q.d_uxy = fresh.back().d_uxy;
    q.d_ufrac = fresh.back().d_ufrac;
    q.need0 = fresh.back().need0;
    q.need1 = fresh.back().need1;
    c->cal.push_back(q);
    union_rows(c);
    *id = (int)c->cal.size() - 1;
    return LT_OK;
}

int lt_calibration_count(lt_ctx* c, int* count) {
    if (!c || !count) return fail(LT_ERR_INVALID, "null argument");
    *count = (int)c->cal.size();
    return LT_OK;
}

int lt_set_slot_calibrations(lt_ctx* c, int first, int n, const int32_t* ids) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (n > 0 && !ids) return fail(LT_ERR_INVALID, "null ids");
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= (int)c->cal.size())
            return fail(LT_ERR_INVALID, "slot %d: calibration set %d out of range (the context has %d)", first + i, ids[i], (int)c->cal.size());
    // Nothing to order on the device: a launch carries the sets of its slots by value.  A slot that changes set has planes made with
    // another set's tables: its front end is stale (lt_mask_rerun).
    for (int i = 0; i < n; ++i) {
        const size_t s = (size_t)(first + i);
        if (c->slot_cal[s] == (uint8_t)ids[i]) continue;
        c->slot_cal[s] = (uint8_t)ids[i];
        front_stale(c, first + i, 1);
    }
    return LT_OK;
}

int lt_get_slot_calibrations(lt_ctx* c, int first, int n, int32_t* ids) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (n > 0 && !ids) return fail(LT_ERR_INVALID, "null ids");
    for (int i = 0; i < n; ++i) ids[i] = slot_set(c, first + i);
    return LT_OK;
}

// ---- compute ------------------------------------------------------------------------------------------
static int mask_run_impl(lt_ctx* c, int first, int n, const lt_filter_params* p, bool reuse_front) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if ((rc = validate_filter(p))) return rc;
    if ((rc = set_device(c))) return rc;
    if (n == 0) return LT_OK;
    // A slot whose surface lt_overlay_run_inplace has drawn into holds no camera frame: only a re-run over planes that are all
    // there is possible (a front end would read the slot's own, stale frame).
    for (int i = first; i < first + n && i < (int)c->drawn.size(); ++i) {
        if (!c->drawn[(size_t)i]) continue;
        bool planes = reuse_front && !c->stage_timing && first + n <= (int)c->front_ok.size();
        for (int j = first; planes && j < first + n; ++j) planes = c->front_ok[(size_t)j] != 0;
        if (!planes)
            return fail(LT_ERR_STATE, "slot %d: its surface was drawn into in place (lt_overlay_run_inplace) and holds no camera frame any more: attach or upload one first", i);
        break;
    }
    const size_t ps = c->masks.plane_bytes;
    const ChainEnv env = chain_env(c);
    if ((rc = raw_sets_ready(c))) return rc;
    c->last_raw_walk_form = 0;
    rc = for_each_slice(c, first, n, [&](hipStream_t st, int f0, int m) {
        // the front end -- unless the caller asked for a RE-run (lt_mask_rerun: the second try of a frame, other filter parameters
        // over the same bird's-eye planes) and these slots' planes are those of the frames they hold
        bool have_front = reuse_front && !c->stage_timing && f0 + m <= (int)c->front_ok.size();
        for (int i = f0; have_front && i < f0 + m; ++i) have_front = c->front_ok[(size_t)i] != 0;
        if (!have_front) {
            // A slice whose slots all have one calibration set -- whichever -- takes the kernels that read one table, with that set's
            // tables; only a slice that mixes sets takes the table-per-slot forms.
            const lt_ctx::CalSet& cs = c->cal[(size_t)slot_set(c, f0)];
            bool mixed = false;
            for (int i = f0 + 1; i < f0 + m && !mixed; ++i) mixed = slot_set(c, i) != slot_set(c, f0);
            { StageScope t(c, ST_UNDISTORT, st);
              // runs of slots whose frames lie in the caller's device memory (the table form) and of slots that hold their own
              auto is_attached = [&](int i) { return i < (int)c->attached.size() && c->attached[(size_t)i] != 0; };
              for (int a = f0, b; a < f0 + m; a = b) {
                  const bool att = is_attached(a);
                  for (b = a + 1; b < f0 + m && is_attached(b) == att; ++b) {}
                  const FrameSource src = att ? FrameSource::surfaces(c->d_surf)
                                          : c->in_layout != LT_INPUT_RGB ? FrameSource::slots(slot_yuv(c, a), c->yuv_stride)
                                                                         : FrameSource::slots(slot_frame(c, a), c->frame_bytes);
                  // One raw set in the run -- whichever -- : today's kernels with that set's stages; several: the set-per-slot forms, which
                  // take the calibration's table per slot as well
                  const RawRun raw = raw_run_of(c, a, b - a);
                  if (raw.one.table) c->last_raw_walk_form = std::max(c->last_raw_walk_form, raw.ids ? 2 : 1);
                  if (mixed || raw.ids) launch_undistort_cal(st, src, c->in_layout, yuv_coef_of(c), c->d_cal, &c->slot_cal[(size_t)a], c->fe, c->d_und, c->und_px, a, b - a, raw.one, raw.sets, raw.ids);
                  else launch_undistort_rows(st, src, c->in_layout, yuv_coef_of(c), cs.d_uxy, cs.d_ufrac, c->fe, c->d_und, c->und_px, a, b - a, raw.one);
              } }
            { int mrc = n == 1 ? note_range_frame(c, c->readers, st, f0, f0 + m) : note_range(c->readers, st, f0, f0 + m); if (mrc) return mrc; }
            { StageScope t(c, ST_WARP_SPLIT, st);
              uint8_t *pr = c->masks.d_plane[P_R] + (size_t)f0 * ps, *pb = c->masks.d_plane[P_B] + (size_t)f0 * ps;
              if (mixed) launch_warp_cal(st, c->d_und, c->und_px, f0, c->d_cal, &c->slot_cal[(size_t)f0], c->fe, c->d_gamma, c->d_cbrt, c->d_coef, pr, pb, ps, m);
              else launch_warp_split(st, c->d_und, c->und_px, f0, cs.d_wxy, cs.d_wfrac, c->fe, c->d_gamma,
                                     c->d_cbrt, c->d_coef, c->lab_clamp_dead, pr, pb, ps, m); }
            for (int i = f0; i < f0 + m && i < (int)c->front_ok.size(); ++i) c->front_ok[(size_t)i] = 1;
        }
        int frc = run_mask_chain(c->masks, env, st, f0, m, p, c->calib.warp_h, c->calib.warp_w, n);
        return frc ? frc : note_written_frame(c, st, f0, f0 + m, n);
    });
    if (rc) return rc;
    c->have_mask = true;
    mark_masks(c, first, n, 1, 0);
    return LT_OK;
}

int lt_mask_run(lt_ctx* c, int first, int n, const lt_filter_params* p) { return mask_run_impl(c, first, n, p, false); }
int lt_mask_rerun(lt_ctx* c, int first, int n, const lt_filter_params* p) { return mask_run_impl(c, first, n, p, true); }

int lt_filter_run(lt_ctx* c, int first, int n, const lt_filter_params* p) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if ((rc = validate_filter(p))) return rc;
    if ((rc = set_device(c))) return rc;
    if (!c->d_bev) return fail(LT_ERR_STATE, "lt_upload_bev has not been called");
    if (n == 0) return LT_OK;
    const size_t ps = c->masks.plane_bytes;
    const ChainEnv env = chain_env(c);
    front_stale(c, first, n);            // the planes become the uploaded bird's-eye image's
    rc = for_each_slice(c, first, n, [&](hipStream_t st, int f0, int m) {
        { StageScope t(c, ST_SPLIT_BEV, st);
          launch_split_bev(st, c->d_bev + (size_t)f0 * c->bev_bytes, c->bev_bytes, (int)ps, c->d_gamma, c->d_cbrt,
                           c->d_coef, c->masks.d_plane[P_R] + (size_t)f0 * ps, c->masks.d_plane[P_B] + (size_t)f0 * ps, ps, m); }
        int frc = run_mask_chain(c->masks, env, st, f0, m, p, c->calib.warp_h, c->calib.warp_w, n);
        return frc ? frc : note_written(c, st, f0, f0 + m);
    });
    if (rc) return rc;
    c->have_mask = true;
    mark_masks(c, first, n, 1, 0);
    return LT_OK;
}

// the range forms' kernels over slots [f0, f0 + m), by their slot addresses (the list form's fallback: one slot at a time)
static void launch_sws_slots(lt_ctx* c, hipStream_t st, const SearchGeom& g, const MaskBits& mb, int f0, int m) {
    launch_sws_fit(st, slot_mask(c, f0), c->masks.plane_bytes, mb, g, slot_band_sums(c, f0, g.nbands), slot_pix(c, f0), slot_cent(c, f0),
                   slot_rec(c, f0), m);
}
static void launch_band_slots(lt_ctx* c, hipStream_t st, const SearchGeom& g, const BandPrev& bp, const MaskBits& mb, int f0, int m) {
    launch_band_fit(st, slot_mask(c, f0), c->masks.plane_bytes, mb, g, slot_prev(c, f0), bp, slot_pix(c, f0), slot_rec(c, f0), m);
}

int lt_sws_fit_run(lt_ctx* c, int first, int n, const lt_search_params* p) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    c->rec_mirror_slot = -1;                  // the records change: the page-locked mirror of a one-frame search is stale
    if ((rc = set_device(c))) return rc;
    if (!c->have_mask) return fail(LT_ERR_STATE, "no mask in the slots: run lt_mask_run or lt_upload_masks first");
    SearchGeom g;
    if ((rc = prepare_search(c, p, false, g))) return rc;
    if (n == 0) return LT_OK;
    const bool use_bits = slot_reads_bits(c, g, 0, first, n);
    if (!use_bits && (rc = ensure_u8_masks(c, first, n))) return rc;
    c->last_search_source = use_bits ? 1 : 0;
    rc = for_each_slice(c, first, n, [&](hipStream_t st, int f0, int m) {
        StageScope t(c, ST_SWS_FIT, st);
        launch_sws_slots(c, st, g, slot_bits(c, f0, use_bits), f0, m);
        if (n == 1) mirror_record(c, st, f0);
        return note_written_frame(c, st, f0, f0 + m, n);
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

int lt_band_fit_run(lt_ctx* c, int first, int n, const lt_search_params* p, const double* prev) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    c->rec_mirror_slot = -1;                  // the records change: the page-locked mirror of a one-frame search is stale
    if (!prev) return fail(LT_ERR_INVALID, "band search needs the previous coefficients (last_left_coeffs/last_right_coeffs)");
    if ((rc = set_device(c))) return rc;
    if (!c->have_mask) return fail(LT_ERR_STATE, "no mask in the slots: run lt_mask_run or lt_upload_masks first");
    SearchGeom g;
    if ((rc = prepare_search(c, p, true, g))) return rc;
    if (n == 0) return LT_OK;
    BandPrev bp;
    std::memset(&bp, 0, sizeof bp);
    bool one_seed = true;     // every frame around the same curves (a group of frames behind a failure: the last valid fits)
    for (int i = 1; i < n && one_seed; ++i) one_seed = std::memcmp(prev, prev + (size_t)i * 6, 6 * sizeof(double)) == 0;
    if (one_seed) {   // the stateful stream: coefficients by value, no copy to wait for
        std::memcpy(bp.c, prev, sizeof bp.c);
        bp.by_value = 1;
    } else {
        if ((rc = sync_all(c))) return rc;
        HIP_TRY(hipMemcpyAsync(slot_prev(c, first), prev, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // prev is caller memory: do not keep reading it after return
    }
    const bool use_bits = slot_reads_bits(c, g, 1, first, n);
    if (!use_bits && (rc = ensure_u8_masks(c, first, n))) return rc;
    c->last_search_source = use_bits ? 1 : 0;
    rc = for_each_slice(c, first, n, [&](hipStream_t st, int f0, int m) {
        StageScope t(c, ST_BAND_FIT, st);
        const MaskBits mb = slot_bits(c, f0, use_bits);
        // one frame (process()): the chain kernel with a chain of one, a third of the latency (LT_BAND_ONE=0: k_band_fit2)
        const char* one_env = n == 1 ? LT_EXP_ENV("LT_BAND_ONE") : nullptr;
        lt_lane_record* mirror = n == 1 ? rec_mirror_device(c) : nullptr;
        unsigned ticket = ++c->rec_ticket_counter;
        if (!ticket) ticket = ++c->rec_ticket_counter;      // 0 means "no ticket"
        if (n == 1 && !(one_env && one_env[0] == '0') &&
            launch_band_fit_one(st, mb, g, bp, slot_pix(c, f0), slot_rec(c, f0), c->masks.plane_bytes, reinterpret_cast<const int*>(c->d_prev),
                                mirror, ticket)) {
            if (mirror) {                    // the kernel itself leaves a copy of the record in page-locked memory, and its ticket
                c->rec_mirror_slot = f0;
                c->rec_mirror_stream = st;
                c->rec_ticket = ticket;
            }
        } else {
            launch_band_slots(c, st, g, bp, mb, f0, m);
            if (n == 1) mirror_record(c, st, f0);
        }
        return note_written_frame(c, st, f0, f0 + m, n);
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

// The searches of a list of frames of unrelated streams (LaneTrackerGroup): one k_search_list launch where its kernels take the
// geometry, else the range forms' kernels slot by slot.  Ordering: the launch goes onto one stream that first waits for the tails of
// every slot stream holding a listed slot (the masks may have been made on any of them) and for the chains touching the slots;
// those slot streams then wait for it, so that whatever is enqueued over these slots later is ordered behind it.
static_assert(sizeof(lt_search_item) == 64, "lt_search_item: 64 bytes, as the header says");
int lt_search_fit_list(lt_ctx* c, int n, const lt_search_item* items, const lt_search_params* sws, const lt_search_params* band) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (n < 0 || (n > 0 && !items)) return fail(LT_ERR_INVALID, "lt_search_fit_list: n < 0 or a null item list");
    int n_sws = 0;
    {
        std::vector<uint8_t> seen((size_t)std::max(c->capacity, 0), 0);
        for (int i = 0; i < n; ++i) {
            const int s = items[i].slot, m = items[i].mode;
            if (s < 0 || s >= c->capacity) return fail(LT_ERR_INVALID, "lt_search_fit_list: item %d: slot %d outside capacity %d", i, s, c->capacity);
            if (seen[(size_t)s]) return fail(LT_ERR_INVALID, "lt_search_fit_list: slot %d listed twice", s);
            if (m != 0 && m != 1) return fail(LT_ERR_INVALID, "lt_search_fit_list: item %d: mode %d (0 sliding window, 1 band)", i, m);
            seen[(size_t)s] = 1;
            n_sws += m == 0;
        }
    }
    if ((n_sws > 0 && !sws) || (n_sws < n && !band)) return fail(LT_ERR_INVALID, "lt_search_fit_list: a parameter set the items need is null");
    if (n == 0) return LT_OK;
    c->rec_mirror_slot = -1;                  // the records change: the page-locked mirror of a one-frame search is stale
    int rc = set_device(c);
    if (rc) return rc;
    if (!c->have_mask) return fail(LT_ERR_STATE, "no mask in the slots: run lt_mask_run or lt_upload_masks first");
    SearchGeom gs, gb;
    std::memset(&gs, 0, sizeof gs);
    std::memset(&gb, 0, sizeof gb);
    if (n_sws > 0 && (rc = prepare_search(c, sws, false, gs))) return rc;
    if (n_sws < n && (rc = prepare_search(c, band, true, gb))) return rc;
    gs.maxpix = gb.maxpix = c->maxpix;        // (the second preparation may have grown the buffers further)
    gs.maxlev = gb.maxlev = c->maxlev;
    // sliding-window items first (k_band_sums_bits runs over the head of the list)
    std::vector<lt_search_item> list(items, items + n);
    std::stable_partition(list.begin(), list.end(), [](const lt_search_item& it) { return it.mode == 0; });
    bool bits = true;
    for (const auto& it : list) bits = bits && masks_have_bits(c, it.slot, 1);
    const bool one_launch = bits && search_list_supported(n_sws > 0 ? &gs : nullptr, n_sws < n ? &gb : nullptr, c->masks.plane_bytes);
    auto geom = [&](const lt_search_item& it) -> const SearchGeom& { return it.mode == 0 ? gs : gb; };
    // (lt_last_search_source: 1 only if no item reads a u8 mask)
    bool all_bits = true;
    if (!one_launch)
        for (const auto& it : list)
            if (!slot_reads_bits(c, geom(it), it.mode, it.slot, 1)) {
                all_bits = false;
                if ((rc = ensure_u8_masks(c, it.slot, 1))) return rc;
            }
    c->last_search_source = all_bits ? 1 : 0;
    // the stream: the urgent one in urgent mode, else the stream of the first listed slot; the other slot streams in front of it
    const int k = slice_count(c);
    std::vector<uint8_t> touched((size_t)k, 0);
    for (const auto& it : list) touched[(size_t)slice_of(c, it.slot)] = 1;
    hipStream_t st = c->urgent_on && c->urgent ? c->urgent : c->streams[(size_t)slice_of(c, list[0].slot)];
    for (int si = 0; si < k; ++si) {
        if (touched[(size_t)si] && c->streams[(size_t)si] != st && (rc = wait_tail(c, st, c->streams[(size_t)si]))) return rc;
    }
    for (const auto& it : list)
        if ((rc = wait_chains(c, st, it.slot, it.slot + 1))) return rc;
    if (one_launch) {
        if (n > c->items_cap) {
            if (c->items_ev) HIP_TRY(hipEventSynchronize(c->items_ev));
            dev_free(c->d_items);
            if (c->h_items) { HIP_TRY(hipHostFree(c->h_items)); c->h_items = nullptr; }
            c->items_cap = 0;
            const int cap = std::max(n, c->capacity);
            if ((rc = dev_alloc(&c->d_items, (size_t)cap))) return rc;
            if (hipHostMalloc(reinterpret_cast<void**>(&c->h_items), (size_t)cap * sizeof(lt_search_item), hipHostMallocDefault) != hipSuccess) {
                c->h_items = nullptr;
                return fail(LT_ERR_HIP, "hipHostMalloc(%zu) failed", (size_t)cap * sizeof(lt_search_item));
            }
            c->items_cap = cap;
        }
        if (!c->items_ev && hipEventCreateWithFlags(&c->items_ev, hipEventDisableTiming) != hipSuccess) return fail(LT_ERR_HIP, "hipEventCreate failed");
        // the previous list's kernels are done with it: items_ev is recorded behind them (below), so neither the staging nor the
        // device copy is overwritten while a search of another call -- on another slot stream, perhaps -- still reads its items
        HIP_TRY(hipEventSynchronize(c->items_ev));
        std::memcpy(c->h_items, list.data(), (size_t)n * sizeof(lt_search_item));
        HIP_TRY(hipMemcpyAsync(c->d_items, c->h_items, (size_t)n * sizeof(lt_search_item), hipMemcpyHostToDevice, st));
        {
            StageScope t(c, n_sws > 0 ? ST_SWS_FIT : ST_BAND_FIT, st);
            // (the whole buffers: the kernel addresses each item's slot itself)
            launch_search_list(st, c->d_items, n, n_sws, c->masks.d_plane[P_MASK], c->masks.plane_bytes, slot_bits(c, 0, true), gs, gb, c->d_band_sums,
                               c->d_pix, c->d_cent, c->d_rec);
        }
        HIP_TRY(hipEventRecord(c->items_ev, st));         // behind the last kernel that reads d_items
    } else {
        for (const auto& it : list) {
            const MaskBits mb = slot_bits(c, it.slot, slot_reads_bits(c, geom(it), it.mode, it.slot, 1));
            if (it.mode == 0) {
                StageScope t(c, ST_SWS_FIT, st);
                launch_sws_slots(c, st, gs, mb, it.slot, 1);
            } else {
                BandPrev bp;
                std::memset(&bp, 0, sizeof bp);
                std::memcpy(bp.c, it.prev_coeffs, sizeof bp.c);
                bp.by_value = 1;
                StageScope t(c, ST_BAND_FIT, st);
                launch_band_slots(c, st, gb, bp, mb, it.slot, 1);
            }
        }
    }
    HIP_TRY(hipGetLastError());
    {   // the writer of exactly the listed slots: one entry per run of consecutive slots
        std::vector<int> slots;
        slots.reserve(list.size());
        for (const auto& it : list) slots.push_back(it.slot);
        std::sort(slots.begin(), slots.end());
        for (size_t a = 0; a < slots.size();) {
            size_t b = a + 1;
            while (b < slots.size() && slots[b] == slots[b - 1] + 1) ++b;
            if ((rc = note_written(c, st, slots[a], slots[b - 1] + 1))) return rc;
            a = b;
        }
    }
    hipEvent_t done = next_order_event(c);
    if (!done) return fail(LT_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(done, st));
    for (int si = 0; si < k; ++si) {
        if (!touched[(size_t)si] || c->streams[(size_t)si] == st) continue;
        HIP_TRY(hipStreamWaitEvent(c->streams[(size_t)si], done, 0));
    }
    return LT_OK;
}

int lt_set_urgent(lt_ctx* c, int on) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    int rc = set_device(c);
    if (rc) return rc;
    if (on && !c->urgent && create_compute_stream(&c->urgent, c->search_cus) != hipSuccess) return fail(LT_ERR_HIP, "hipStreamCreate failed");
    if (!on && c->urgent_on && c->urgent) HIP_TRY(hipStreamSynchronize(c->urgent));   // leaving: nothing of it is left in flight unseen
    c->urgent_on = on != 0;
    return LT_OK;
}

int lt_set_walk_min_frames(lt_ctx* c, int frames) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    c->walk_min_pixels = frames < 0 ? 80LL * 1100 * 1080 : (long long)frames * c->calib.warp_w * c->calib.warp_h;
    return LT_OK;
}

int lt_set_search_cus(lt_ctx* c, int n) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (n < 0 || n > 64) return fail(LT_ERR_INVALID, "the search stream can have 0 .. 64 CUs to itself");
    int rc = set_device(c);
    if (rc) return rc;
    if (n == c->search_cus) return LT_OK;
    if ((rc = sync_all(c))) return rc;
    if ((rc = flush_stage_events(c))) return rc;
    // every stream that carries slot kernels is recreated with (or without) the reservation; the search stream follows on its
    // next use
    std::vector<hipStream_t> fresh;
    for (size_t i = 0; i < c->streams.size(); ++i) {
        hipStream_t st = nullptr;
        if (create_compute_stream(&st, n) != hipSuccess) {
            for (auto f : fresh) stream_put(f);
            return fail(LT_ERR_HIP, "stream with a CU mask could not be created");
        }
        fresh.push_back(st);
    }
    for (auto st : c->streams) stream_put(st);
    c->streams = fresh;
    c->stream = c->streams.empty() ? c->stream : c->streams[0];
    stream_put(c->search); c->search = nullptr;
    stream_put(c->present); c->present = nullptr;
    stream_put(c->urgent); c->urgent = nullptr; c->urgent_on = false;
    stream_put(c->dl); c->dl = nullptr;
    c->search_cus = n;
    c->rec_mirror_slot = -1;             // the stream the mirror of a one-frame search was queued on is gone
    c->rec_mirror_stream = nullptr;
    return LT_OK;
}

// ---- host-buffer wrappers --------------------------------------------------------------------------------
int lt_mask_batch(lt_ctx* c, const uint8_t* frames, int n, const lt_filter_params* p, uint8_t* masks) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    int rc;
    if (n > c->capacity && (rc = lt_reserve(c, n))) return rc;
    if ((rc = lt_upload_frames(c, frames, 0, n))) return rc;
    if ((rc = lt_mask_run(c, 0, n, p))) return rc;
    return lt_download_masks(c, 0, n, masks);
}

int lt_sws_fit_batch(lt_ctx* c, const uint8_t* masks, int n, const lt_search_params* p, lt_lane_record* out) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    int rc;
    if (n > c->capacity && (rc = lt_reserve(c, n))) return rc;
    if (masks && (rc = lt_upload_masks(c, masks, 0, n))) return rc;
    if ((rc = lt_sws_fit_run(c, 0, n, p))) return rc;
    return lt_download_records(c, 0, n, out);
}

int lt_band_fit_batch(lt_ctx* c, const uint8_t* masks, int n, const lt_search_params* p, const double* prev,
                      lt_lane_record* out) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    int rc;
    if (n > c->capacity && (rc = lt_reserve(c, n))) return rc;
    if (masks && (rc = lt_upload_masks(c, masks, 0, n))) return rc;
    if ((rc = lt_band_fit_run(c, 0, n, p, prev))) return rc;
    return lt_download_records(c, 0, n, out);
}

// ---- single-image operators ------------------------------------------------------------------------------
int lt_bilateral_adaptive_threshold(lt_ctx* c, const uint8_t* img, int h, int w, int ksize, int C, int mode, int tv,
                                    int fv, uint8_t* out) {
    if (!c || !img || !out) return fail(LT_ERR_INVALID, "null argument");
    if (mode != 0 && mode != 1) return fail(LT_ERR_INVALID, "Unexpected mode value. Expected value is 'floor' or 'ceil'.");
    if (h < 1 || w < 1 || ksize < 1 || ksize > 128) return fail(LT_ERR_INVALID, "bad image size or ksize (1..128)");
    if (tv < 0 || tv > 255 || fv < 0 || fv > 255) return fail(LT_ERR_INVALID, "true/false values must be in [0,255]");
    int rc = set_device(c);
    if (rc) return rc;
    const size_t n = (size_t)h * w;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    if ((rc = dev_alloc(&d_in, n))) return rc;
    if ((rc = dev_alloc(&d_out, n))) { dev_free(d_in); return rc; }
    hipError_t e = hipMemcpyAsync(d_in, img, n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_bilateral(c->stream, d_in, d_out, h, w, ksize, C, mode, tv, fv, n, 1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(d_in);
    dev_free(d_out);
    if (e != hipSuccess) return fail(LT_ERR_HIP, "bilateral threshold failed: %s", hipGetErrorString(e));
    return LT_OK;
}

// ---- one host frame -> RGB, on the device ---------------------------------------------------------------------------------------------
// (convert_once and the raw Bayer converters: lt_raw.cpp)
// one 4:2:0 host frame of any even size (h w 3 / 2 bytes), or one packed 4:2:2 frame of any even width (h w 2 bytes) -> RGB
// (cv2.cvtColor(frame, COLOR_YUV2RGB_NV12 / _I420 / _YUY2 / _UYVY) with the given matrix)
int lt_yuv_to_rgb(lt_ctx* c, const uint8_t* frame, int h, int w, int layout, const int32_t* coeffs, uint8_t* out_rgb) {
    if (!c || !frame || !out_rgb) return fail(LT_ERR_INVALID, "null argument");
    int rc = check_yuv_format(layout, coeffs, h, w);
    if (rc) return rc;
    if ((rc = check_one_shot_size(layout, h, w))) return rc;
    const size_t px = (size_t)h * w;
    RawSetup none;
    none.layout = layout;
    return convert_once(c, "YUV conversion", frame, is_422(layout) ? px * 2 : px * 3 / 2, h, w, YuvCoef{coeffs[0], coeffs[1], coeffs[2], coeffs[3], coeffs[4]}, none,
                        out_rgb);
}

int lt_filter_lane_points(lt_ctx* c, const uint8_t* bev, int h, int w, const lt_filter_params* p, uint8_t* mask) {
    if (!c || !bev || !mask) return fail(LT_ERR_INVALID, "null argument");
    int rc = validate_filter(p);
    if (rc) return rc;
    if (h < 1 || w < 1 || h > 16384 || w > 4096) return fail(LT_ERR_INVALID, "bad image size (width <= 4096, height <= 16384)");
    if ((rc = set_device(c))) return rc;
    // a private one-slot arena of the requested size (the image may differ from the calibration's BEV size): whatever the chain
    // allocates in it is freed with it, when this call returns
    MaskArena arena;
    arena.set_geometry(h, w);
    const size_t ps = arena.plane_bytes;
    uint8_t* d_bev = nullptr;
    if ((rc = arena.reserve(1, false)) || (rc = dev_alloc(&d_bev, ps * 3))) return rc;
    const ChainEnv env{&c->se29, &c->se55, c->brute_tophat};   // no batch kernels, no stage timing, nobody asks for the route
    hipError_t e = hipMemcpyAsync(d_bev, bev, ps * 3, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_split_bev(c->stream, d_bev, ps * 3, (int)ps, c->d_gamma, c->d_cbrt, c->d_coef, arena.d_plane[P_R], arena.d_plane[P_B], ps, 1);
        rc = run_mask_chain(arena, env, c->stream, 0, 1, p, h, w, 1, true);
        if (rc == LT_OK) e = hipMemcpyAsync(mask, arena.d_plane[P_MASK], ps, hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(d_bev);
    if (rc) return rc;
    if (e != hipSuccess) return fail(LT_ERR_HIP, "filter_lane_points failed: %s", hipGetErrorString(e));
    return LT_OK;
}

int lt_morph_ellipse(lt_ctx* c, const uint8_t* img, int h, int w, int k, int op, int direct, uint8_t* out) {
    if (!c || !img || !out) return fail(LT_ERR_INVALID, "null argument");
    if (h < 1 || w < 1 || h > 16384 || w > 16384) return fail(LT_ERR_INVALID, "bad image size");
    if (k != 5 && k != 29 && k != 55) return fail(LT_ERR_INVALID, "structuring element size must be 5, 29 or 55");
    if (op < 0 || op > 3) return fail(LT_ERR_INVALID, "op must be 0 erode, 1 dilate, 2 tophat, 3 open");
    int rc = set_device(c);
    if (rc) return rc;
    const size_t n = (size_t)h * w;
    uint8_t *d_in = nullptr, *d_t = nullptr, *d_out = nullptr;
    if ((rc = dev_alloc(&d_in, n)) || (rc = dev_alloc(&d_t, n)) || (rc = dev_alloc(&d_out, n))) {
        dev_free(d_in); dev_free(d_t); dev_free(d_out);
        return rc;
    }
    const EllipseSE& se = k == 5 ? c->se5 : (k == 29 ? c->se29 : c->se55);
    auto pass = [&](const uint8_t* src, uint8_t* dst, const uint8_t* minuend, bool dilate) {
        if (k == 5 || direct) launch_morph_ellipse(c->stream, src, dst, minuend, h, w, se, dilate, n, 1);
        else launch_morph_runs(c->stream, src, dst, minuend, h, w, k, dilate, n, 1);
    };
    hipError_t e = hipMemcpyAsync(d_in, img, n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        if (op == 0) pass(d_in, d_out, nullptr, false);
        else if (op == 1) pass(d_in, d_out, nullptr, true);
        else { pass(d_in, d_t, nullptr, false); pass(d_t, d_out, op == 2 ? d_in : nullptr, true); }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(d_in); dev_free(d_t); dev_free(d_out);
    if (e != hipSuccess) return fail(LT_ERR_HIP, "morph_ellipse failed: %s", hipGetErrorString(e));
    return LT_OK;
}

// Test hook: ONE call of the top-hat launchers (k_tophat.hip) on planes given by value, in buffers of this call's own.  The destination,
// the intermediate and the copy plane are n + 2 planes each, 0xA5 everywhere before the launch; the work goes to planes 1 .. n, so a
// store outside them -- the pitch padding, the plane before, the PAIR strip's "frame n" behind -- comes back to the caller.
int lt_morph_planes(lt_ctx* c, const uint8_t* planes, int n, int h, int w, int k, int op, int bands, int dpitch, int route,
                    uint8_t* dst_out, uint8_t* mid_out, uint8_t* copy_out, lt_morph_report* report, int* launched) {
    if (!c || !planes || !dst_out || !report || !launched) return fail(LT_ERR_INVALID, "null argument");
    if (h < 1 || w < 1 || h > 4096 || w > 4096 || n < 1 || n > 16) return fail(LT_ERR_INVALID, "lt_morph_planes: 1 .. 16 planes of at most 4096 x 4096");
    if (k != 29 && k != 55) return fail(LT_ERR_INVALID, "structuring element size must be 29 or 55");
    if (op < 0 || op > 3) return fail(LT_ERR_INVALID, "op must be 0 erode, 1 dilate, 2 top-hat, 3 top-hat with minuend copy");
    if (route != 0 && route != 1) return fail(LT_ERR_INVALID, "route must be 0 (launch_morph_runs) or 1 (launch_morph_one_pair)");
    if (route == 1 && (n > 2 || op == 3)) return fail(LT_ERR_INVALID, "the pair launch takes one or two frames and has no minuend copy");
    if (bands < 0 || (dpitch != 0 && dpitch != ((w + 63) & ~63))) return fail(LT_ERR_INVALID, "bands >= 0; dpitch is 0 or the width rounded up to 64");
    if ((op >= 2) && !mid_out) return fail(LT_ERR_INVALID, "a top-hat returns its eroded intermediate: mid_out is null");
    if (op == 3 && !copy_out) return fail(LT_ERR_INVALID, "copy_out is null");
    int rc = set_device(c);
    if (rc) return rc;
    std::memset(report, 0, sizeof *report);
    *launched = 0;
    const int sets = route == 1 ? 2 : 1;                    // route 1: the 55x55 chain's planes, then the 29x29 chain's
    const size_t ps = (size_t)h * w, pitch = dpitch ? (size_t)dpitch : (size_t)w, ds = (size_t)h * pitch;
    const size_t src_bytes = (size_t)sets * n * ps, mid_bytes = (size_t)sets * (n + 2) * ps, dst_bytes = (size_t)sets * (n + 2) * ds;
    DevBuf<uint8_t> d_src, d_mid, d_dst, d_copy;
    DevBuf<uint32_t> d_zone;
    MorphZone zone;
    if ((rc = d_src.alloc(src_bytes)) || (rc = d_mid.alloc(mid_bytes)) || (rc = d_dst.alloc(dst_bytes)) || (rc = d_copy.alloc(dst_bytes))) return rc;
    if (route == 0 && n > 2) {   // as MaskArena sizes it (set_geometry, ensure_zone_scratch): the 55x55 zones, per frame and strip
        zone.stride_dwords = (size_t)((w + 127) / 128) * tophat_split_zone_dwords(55);
        if ((rc = d_zone.alloc((size_t)n * zone.stride_dwords))) return rc;
        zone.base = d_zone.p;
    }
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d_src.p, planes, src_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_mid.p, 0xA5, mid_bytes, s));
    HIP_TRY(hipMemsetAsync(d_dst.p, 0xA5, dst_bytes, s));
    HIP_TRY(hipMemsetAsync(d_copy.p, 0xA5, dst_bytes, s));
    MorphReport rep;
    bool ok = true;
    if (route == 0) {
        uint8_t *mid = d_mid.p + ps, *dst = d_dst.p + ds, *cp = d_copy.p + ds;
        if (op == 0) ok = launch_morph_runs(s, d_src.p, dst, nullptr, h, w, k, false, ps, n, dpitch, ds, nullptr, zone, nullptr, bands, &rep);
        else if (op == 1) ok = launch_morph_runs(s, d_src.p, dst, nullptr, h, w, k, true, ps, n, dpitch, ds, nullptr, zone, nullptr, bands, &rep);
        else {
            ok = launch_morph_runs(s, d_src.p, mid, nullptr, h, w, k, false, ps, n, 0, 0, nullptr, zone, nullptr, bands, &rep);
            if (ok) ok = launch_morph_runs(s, mid, dst, d_src.p, h, w, k, true, ps, n, dpitch, ds, op == 3 ? cp : nullptr, zone, nullptr, bands, &rep);
        }
    } else {
        const uint8_t *s55 = d_src.p, *s29 = d_src.p + (size_t)n * ps;
        uint8_t *m55 = d_mid.p + ps, *m29 = d_mid.p + (size_t)(n + 2) * ps + ps, *o55 = d_dst.p + ds, *o29 = d_dst.p + (size_t)(n + 2) * ds + ds;
        if (op == 0) ok = launch_morph_one_pair(s, s55, o55, nullptr, s29, o29, nullptr, h, w, false, ps, n, dpitch, ds, bands, &rep);
        else if (op == 1) ok = launch_morph_one_pair(s, s55, o55, nullptr, s29, o29, nullptr, h, w, true, ps, n, dpitch, ds, bands, &rep);
        else {
            ok = launch_morph_one_pair(s, s55, m55, nullptr, s29, m29, nullptr, h, w, false, ps, n, 0, 0, bands, &rep);
            if (ok) ok = launch_morph_one_pair(s, m55, o55, s55, m29, o29, s29, h, w, true, ps, n, dpitch, ds, bands, &rep);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst_out, d_dst.p, dst_bytes, hipMemcpyDeviceToHost, s));
    if (mid_out) HIP_TRY(hipMemcpyAsync(mid_out, d_mid.p, mid_bytes, hipMemcpyDeviceToHost, s));
    if (copy_out) HIP_TRY(hipMemcpyAsync(copy_out, d_copy.p, dst_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *launched = ok ? 1 : 0;
    report->family = ok ? rep.family : 0;
    report->wide = rep.wide;
    report->nbands = rep.nbands;
    report->band_rows = rep.band_rows;
    report->pair_strip = rep.pair_strip;
    report->q = rep.q;
    report->nbands29 = rep.nbands29;
    report->band_rows29 = rep.band_rows29;
    return LT_OK;
}

int lt_fit_poly2(lt_ctx* c, const int32_t* ys, const int32_t* xs, int n, int h, int w, double coef[3], int* rank_deficient) {
    if (!c || !coef || !rank_deficient || n < 0 || (n > 0 && (!ys || !xs))) return fail(LT_ERR_INVALID, "bad argument");
    if (h < 1 || w < 1) return fail(LT_ERR_INVALID, "bad image size");
    int rc = set_device(c);
    if (rc) return rc;
    std::vector<uint32_t> packed((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (ys[i] < 0 || ys[i] > 65535 || xs[i] < 0 || xs[i] > 65535) return fail(LT_ERR_INVALID, "pixel coordinate outside [0, 65535]");
        packed[i] = ((uint32_t)ys[i] << 16) | (uint32_t)xs[i];
    }
    uint32_t* d_pix = nullptr;
    double* d_out = nullptr;
    if ((rc = dev_alloc(&d_pix, (size_t)n))) return rc;
    if ((rc = dev_alloc(&d_out, 4))) { dev_free(d_pix); return rc; }
    double out[4] = {0, 0, 0, 1};
    hipError_t e = n ? hipMemcpyAsync(d_pix, packed.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    if (e == hipSuccess) {
        launch_fit_list(c->stream, d_pix, n, h, w, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(d_pix);
    dev_free(d_out);
    if (e != hipSuccess) return fail(LT_ERR_HIP, "fit_poly2 failed: %s", hipGetErrorString(e));
    coef[0] = out[0]; coef[1] = out[1]; coef[2] = out[2];
    *rank_deficient = out[3] != 0.0;
    return LT_OK;
}

// ---- measurement ---------------------------------------------------------------------------------------
int lt_timer_start(lt_ctx* c) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    { int rc = sync_all(c); if (rc) return rc; }
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    return LT_OK;
}

int lt_timer_stop(lt_ctx* c, float* ms) {
    if (!c || !ms) return fail(LT_ERR_INVALID, "null argument");
    { int rc = sync_all(c); if (rc) return rc; }
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return LT_OK;
}

int lt_last_threshold_path(lt_ctx* c) {
    if (!c) { (void)fail(LT_ERR_INVALID, "null context"); return LT_NO_CONTEXT; }
    return c->last_threshold_path;
}

int lt_last_threshold_form(lt_ctx* c) {
    if (!c) { (void)fail(LT_ERR_INVALID, "null context"); return LT_NO_CONTEXT; }
    return c->last_threshold_form;
}

int lt_last_open_form(lt_ctx* c) {
    if (!c) { (void)fail(LT_ERR_INVALID, "null context"); return LT_NO_CONTEXT; }
    return c->last_open_form;
}

int lt_last_search_source(lt_ctx* c) {
    if (!c) { (void)fail(LT_ERR_INVALID, "null context"); return LT_NO_CONTEXT; }
    return c->last_search_source;
}

int lt_last_tophat_path(lt_ctx* c) {
    if (!c) { (void)fail(LT_ERR_INVALID, "null context"); return LT_NO_CONTEXT; }
    return c->last_tophat_path;
}

int lt_last_overlay_launches(lt_ctx* c) {
    if (!c) { (void)fail(LT_ERR_INVALID, "null context"); return LT_NO_CONTEXT; }
    return c->last_overlay_launches;
}

int lt_tophat_split_form(int h, int w, int k, int nbands) {
    if (h <= 0 || w <= 0 || nbands <= 0) return 0;
    const int band_rows = (h + nbands - 1) / nbands;
    return lt::tophat_split_form(h, w, k, band_rows, (h + band_rows - 1) / band_rows, (w & 3) == 0 && w >= 4) ? 1 : 0;
}

int lt_last_adaptive_path(lt_ctx* c) {
    if (!c) { (void)fail(LT_ERR_INVALID, "null context"); return LT_NO_CONTEXT; }
    return c->last_adaptive_path;
}

int lt_set_stage_timing(lt_ctx* c, int enabled) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    int rc = flush_stage_events(c);
    c->stage_timing = enabled != 0;
    return rc;
}

int lt_stage_reset(lt_ctx* c) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    int rc = flush_stage_events(c);
    std::memset(c->stage_ms, 0, sizeof c->stage_ms);
    std::memset(c->stage_launches, 0, sizeof c->stage_launches);
    return rc;
}

int lt_stage_ms(lt_ctx* c, float* ms, int32_t* launches, int n) {
    if (!c || !ms) return fail(LT_ERR_INVALID, "null argument");
    int rc = flush_stage_events(c);
    for (int i = 0; i < n && i < LT_NUM_STAGES; ++i) {
        ms[i] = c->stage_ms[i];
        if (launches) launches[i] = c->stage_launches[i];
    }
    return rc;
}

}  // extern "C"

namespace lt {
int set_error(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
int ctx_device(lt_ctx* c) { return c->device; }
int ctx_streams(lt_ctx* c, hipStream_t* out, int cap) {
    int n = 0;
    for (int i = 0; i < c->nstreams && i < (int)c->streams.size() && n < cap; ++i) out[n++] = c->streams[(size_t)i];
    return n;
}
int ctx_sync(lt_ctx* c) { return lt_sync(c); }
int ctx_enqueue_records(lt_ctx* c, int first, int n, lt_lane_record* dst) { return lt_enqueue_records_to_device(c, first, n, dst); }
}  // namespace lt