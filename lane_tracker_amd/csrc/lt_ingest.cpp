// Host frames into the slots of liblane_tracker_amd.so: lt_upload_frames, the lt_upload_frame_rows family, lt_upload_frame_rest /
// _rest_rows, their pointer-list forms and lt_device_frames_rest.  A frame reaches a slot in one of three ways -- direct, staged or
// resized -- and the way is a value (Ingest, from ingest_of): every entry point is written once over it.  DESIGN.md section 3 holds
// the table entry point x kind: rows copied and to where, stream, waits before, kernel behind, notes after.  See lt_ctx.h.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <immintrin.h>
#include <sys/mman.h>
#include <unistd.h>

#include "bayer_arith.h"
#include "lt_ctx.h"

using namespace lt;

namespace {

// Rows of a caller's frame: [r0, r1) of its first (or only) plane and -- planar 4:2:0 -- rows [c0, c1) of its chroma plane(s).
struct Rows { int r0, r1, c0, c1; };
// chroma rows under the Y rows [r0, r1)
inline int chroma_lo(int r0) { return r0 / 2; }
inline int chroma_hi(int r0, int r1) { return r1 > r0 ? (r1 - 1) / 2 + 1 : r0 / 2; }

// Rows [r0, r1) of the Y plane and rows [c0, c1) of the chroma plane(s) of n host frames (yuv_bytes apart) into the staging
// frames of slots [first, first + n), on `st`: one pitched copy per plane piece.
int yuv_copy(lt_ctx* c, const uint8_t* frames, int first, int n, int r0, int r1, int c0, int c1, hipStream_t st) {
    const size_t W = (size_t)c->calib.img_w, plane = (size_t)c->calib.img_h * W;
    uint8_t* dst = slot_yuv(c, first);
    auto piece = [&](size_t off, size_t bytes) {
        HIP_TRY(hipMemcpy2DAsync(dst + off, c->yuv_stride, frames + off, c->yuv_bytes, bytes, (size_t)n, hipMemcpyHostToDevice, st));
        return (int)LT_OK;
    };
    int rc = LT_OK;
    if (const size_t row = (size_t)one_plane_row_bytes(c->in_layout, c->calib.img_w))   // one plane of 2 W (4:2:2), 3 W (BGR), 4 W (RGBA / BGRA) ... bytes a row: its rows [r0, r1); no chroma rows
        return r1 > r0 ? piece((size_t)r0 * row, (size_t)(r1 - r0) * row) : rc;
    if (r1 > r0 && c1 > c0 && r0 == 0 && r1 == c->calib.img_h && c0 == 0 && c1 == c->calib.img_h / 2) return piece(0, c->yuv_bytes);
    if (r1 > r0 && (rc = piece((size_t)r0 * W, (size_t)(r1 - r0) * W))) return rc;
    if (c1 <= c0) return rc;
    if (c->in_layout == LT_INPUT_NV12) return piece(plane + (size_t)c0 * W, (size_t)(c1 - c0) * W);
    if ((rc = piece(plane + (size_t)c0 * (W / 2), (size_t)(c1 - c0) * (W / 2)))) return rc;
    return piece(plane + plane / 4 + (size_t)c0 * (W / 2), (size_t)(c1 - c0) * (W / 2));
}

// Frames of another size (lt_set_input_size): which source rows a run of camera rows reads follows from the vertical tap table
// (resize_arith.h: input_run).
void rs_input_rows(const lt_ctx* c, int a, int b, int* s0, int* s1) {
    if (b <= a) { *s0 = *s1 = 0; return; }
    *s0 = c->rs_yt[4 * (size_t)a];
    *s1 = c->rs_yt[4 * (size_t)(b - 1) + 1] + 1;
}

// How the frames of this context's caller reach a slot: the kind, and everything the entry points below differ in by kind.
//   direct   plain RGB of the calibration's size: rows straight into the slot's RGB camera frame, which everything reads
//   staged   every other pixel format: rows into the slot's staging frame (slot_yuv), which the undistortion reads; the row
//            conversion fills the RGB camera frame for whoever shows it
//   resized  RGB of another size: source rows into slot_src, and the resize fills the camera frame, which the undistortion reads
struct Ingest {
    enum Kind { DIRECT, STAGED, RESIZED };
    lt_ctx* c;
    Kind kind;
    size_t frame_pitch;         // bytes between the caller's frames: frame_bytes, yuv_bytes or src_bytes
    bool staging;               // the copies land in a staging frame that finish() reads: a rest's finish waits for the enqueued row uploads
                                // into it (yuv_rows) and is noted as a reader of the slots (the next upload into staging waits for it)
    bool front_reads_staging;   // the undistortion reads the staging frame itself: a row upload for the path finishes nothing
    Rows path;                  // the rows of the caller's frame that the path's upload brings ({0, 0, 0, 0}: none)
    int made0, made1;           // the camera rows that upload has made in the RGB camera frame (a rest makes the others): none where it finishes nothing

    // The rows of the caller's frame that camera rows [a, b) need: for the path, or -- `shown` -- for the RGB camera frame.
    Rows rows_for(int a, int b, bool shown) const {
        const int H = c->calib.img_h;
        if (kind == RESIZED) {
            if (shown && a == 0 && b == H) return Rows{0, c->src_h, 0, 0};     // the whole camera frame takes the whole source frame
            Rows r{0, 0, 0, 0};
            rs_input_rows(c, a, b, &r.r0, &r.r1);
            return r;
        }
        if (kind == STAGED && is_raw_mosaic(c->in_layout) && b > a) {
            // raw Bayer: the rows the taps' windows touch (the path), or the rows the demosaic of the run reads (shown)
            if (shown) ba::support_run(a, b, H, &a, &b);
            else ba::input_run(a, b, H, &a, &b);
        }
        return kind == STAGED ? Rows{a, b, chroma_lo(a), chroma_hi(a, b)} : Rows{a, b, 0, 0};
    }

    // Rows r of n host frames into slots [first, first + n), on `st`.
    int copy(const uint8_t* frames, int first, int n, const Rows& r, hipStream_t st) const {
        if (r.r1 <= r.r0) return LT_OK;
        if (kind == STAGED) return yuv_copy(c, frames, first, n, r.r0, r.r1, r.c0, r.c1, st);
        // (one frame, measured in round 5 against this pitched copy, 279-286 us per frame of process(): a plain copy of the contiguous
        // run 315-320; the rows onto page-locked staging by the copy threads and an asynchronous engine copy from there 295-329, a copy
        // kernel from there 320 -- the runtime's pageable path is the fastest of the four.  The rows in two to four pieces, so that the
        // engine's copy of one runs under the runtime's staging of the next: measured SLOWER, 195-218 against 183-186 us per 1280x720
        // frame -- every piece pays the call again; NOTES_r06 E.2)
        const bool rs = kind == RESIZED;
        const size_t rb = (size_t)(rs ? c->src_w : c->calib.img_w) * 3, off = (size_t)r.r0 * rb, bytes = (size_t)(r.r1 - r.r0) * rb;
        uint8_t* dst = (rs ? slot_src(c, first) : slot_frame(c, first)) + off;
        if (!rs && bytes == c->frame_bytes)          // whole frames back to back on both sides: one flat copy
            HIP_TRY(hipMemcpyAsync(dst, frames, (size_t)n * c->frame_bytes, hipMemcpyHostToDevice, st));
        else
            HIP_TRY(hipMemcpy2DAsync(dst, rs ? c->src_stride : c->frame_bytes, frames + off, frame_pitch, bytes, (size_t)n, hipMemcpyHostToDevice, st));
        return LT_OK;
    }
    // ... the rows that shown camera rows [a, b) need and the path's upload has not brought: what lies below its run, and above it
    int copy_rest(const uint8_t* frames, int first, int n, int a, int b, hipStream_t st) const {
        const Rows r = rows_for(a, b, true);
        const int rc = copy(frames, first, n, Rows{r.r0, std::min(r.r1, path.r0), r.c0, std::min(r.c1, path.c0)}, st);
        return rc ? rc : copy(frames, first, n, Rows{std::max(r.r0, path.r1), r.r1, std::max(r.c0, path.c1), r.c1}, st);
    }

    // Camera rows [a, b) of the RGB camera frames of slots [first, first + n) from what was copied, on `st`.
    int finish(hipStream_t st, int first, int n, int a, int b) const {
        if (kind == STAGED) {
            if (int rc = raw_sets_ready(c)) return rc;
            const RawRun raw = raw_run_of(c, first, n);
            launch_yuv_rows_to_rgb(st, c->in_layout, slot_yuv(c, first), c->yuv_stride, yuv_coef_of(c), slot_frame(c, first), c->frame_bytes,
                                   c->calib.img_h, c->calib.img_w, a, b, n, raw.one, raw.sets, raw.ids);
        } else if (kind == RESIZED)
            launch_resize_rows(st, slot_src(c, first), c->src_stride, c->src_bytes, c->src_w, slot_frame(c, first), c->frame_bytes, c->calib.img_w,
                               a, b, c->d_rs_xt, c->d_rs_yt, n);
        else
            return LT_OK;
        HIP_TRY(hipGetLastError());
        return LT_OK;
    }

    // What an enqueued upload of the path's rows into slots [f0, f0 + m), on their own stream `st`, leaves for later calls to wait for.
    int note_enqueued(hipStream_t st, int f0, int m) const;
};

// The only place that asks the context which way its host frames go.
Ingest ingest_of(lt_ctx* c) {
    Ingest in{};
    in.c = c;
    in.kind = c->in_layout != LT_INPUT_RGB ? Ingest::STAGED : resizes(c) ? Ingest::RESIZED : Ingest::DIRECT;
    in.frame_pitch = in.kind == Ingest::STAGED ? c->yuv_bytes : in.kind == Ingest::RESIZED ? c->src_bytes : c->frame_bytes;
    in.staging = in.kind != Ingest::DIRECT;
    in.front_reads_staging = in.kind == Ingest::STAGED;
    const bool reads = c->cam_r1 > c->cam_r0;
    in.path = reads ? in.rows_for(c->cam_r0, c->cam_r1, false) : Rows{0, 0, 0, 0};
    if (in.path.r1 <= in.path.r0) in.path = Rows{0, 0, 0, 0};
    in.made0 = reads && !in.front_reads_staging ? c->cam_r0 : 0;
    in.made1 = reads && !in.front_reads_staging ? c->cam_r1 : 0;
    return in;
}

// The preamble of the uploads of camera rows into slots [first, first + n): slots and frames valid; the device current when there
// is anything to copy.
int check_upload(lt_ctx* c, const uint8_t* frames, int first, int n) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (!frames) return fail(LT_ERR_INVALID, "null frames");
    if (n > 0) c->input_locked = true;
    detach_slots(c, first, n);
    return n > 0 ? set_device(c) : LT_OK;
}

// ---- one frame's rows through the PCIe aperture ----------------------------------------------------------------------------------
// With a large BAR the whole device memory is mapped into the process, write-combining, at the addresses hipMalloc hands out: the
// calling thread can store a frame's rows into the slot itself.  For the ONE frame of a LaneTracker.process() call that beats the
// copy engine: hipMemcpy2DAsync costs the call 8-24 us (by box) before the engine even starts (23 us of copy + 6 us until the
// first kernel behind it), the stores take the bus's 20 us for the 914 KB of a 1280x720 frame's rows and the undistortion can be
// launched the moment they are out (tools/microbench/upload_latency.hip: rows out of cold memory + a dependent kernel 66 -> 43 us;
// NOTES_r06 E.6 for the frame).  The bytes are the same bytes; only their way differs.
// Ordering: the stores end with an sfence and are posted writes of the thread that then rings the launch's doorbell (or of
// threads it has waited for); the kernels behind them start with an acquire that drops what the XCDs' L2s still hold of the
// slot's previous frame (as between any two kernels), and the memory-side cache sees the bus's writes.  In front: nothing is
// waited for -- the aperture is taken only when the library already KNOWS the slot's readers are done (camera_rows_known_idle).
// Up to 1.5 MB per call: the 914 KB of a 1280x720 frame's rows take the calling thread (and two polling copy threads) 25 us against
// the engine's 8 + 29 us; the 2.0 MB of a 1920x1080 frame's take them 52-60 us against the engine's 9 + 51 us, most of which the
// engine spends beside the mask chain's launches -- no gain there, and a busy host (tools/process_points.py, NOTES_r06 E.6).
constexpr size_t APERTURE_MAX_BYTES = (size_t)3 << 19;
bool host_has_mapped(const void* p, size_t n) {
    const uintptr_t pg = (uintptr_t)sysconf(_SC_PAGESIZE);
    unsigned char v = 0;
    auto mapped = [&](uintptr_t a) { return mincore((void*)(a & ~(pg - 1)), 1, &v) == 0; };
    return n > 0 && mapped((uintptr_t)p) && mapped((uintptr_t)p + n - 1);
}
bool direct_upload_possible(lt_ctx* c) {
    if (c->direct_upload < 0)
        c->direct_upload = c->prop.isLargeBar && c->d_frames && host_has_mapped(c->d_frames, (size_t)c->capacity * c->frame_bytes) ? 1 : 0;
    return c->direct_upload == 1 && c->direct_upload_wanted && ingest_of(c).kind == Ingest::DIRECT;   // (staged frames take the engine; so do frames of another size: their rows go to staging)
}
__attribute__((target("avx2"))) void store_stream_avx2(uint8_t* dst, const uint8_t* src, size_t n) {
    size_t head = (32 - ((uintptr_t)dst & 31)) & 31;
    if (head > n) head = n;
    if (head) { std::memcpy(dst, src, head); dst += head; src += head; n -= head; }
    size_t i = 0;
    for (; i + 128 <= n; i += 128) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i));
        const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i + 32));
        const __m256i d = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i + 64));
        const __m256i e = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i + 96));
        _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i), a);
        _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 32), b);
        _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 64), d);
        _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 96), e);
    }
    if (i < n) std::memcpy(dst + i, src + i, n - i);
}
void store_piece(uint8_t* dst, const uint8_t* src, size_t n) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) store_stream_avx2(dst, src, n);
    else std::memcpy(dst, src, n);
    _mm_sfence();
}
// One thread moves a frame's rows at what it can READ from memory the caller's frame lies cold in (30 us for 914 KB); two or three
// reach the bus's 20 us (tools/microbench/upload_latency.hip, COLD=1).  The copy threads that are polling for work at this moment
// (LaneTracker.process() keeps two or three of them warm with the rows of its output frames) are offered a piece each; pieces
// nobody has claimed when the calling thread is through with its own are the calling thread's again -- no piece waits for a
// sleeper, and none for a queue another tracker has filled.
void store_through_aperture(uint8_t* dst, const uint8_t* src, size_t n) {
    const int helpers = n >= ((size_t)256 << 10) ? std::min(host_copy_pollers(), 2) : 0;
    if (helpers <= 0) { store_piece(dst, src, n); return; }
    struct Split {
        std::atomic<int> claimed[3];
        std::atomic<int> done{0};
        uint8_t* dst; const uint8_t* src; size_t lo[4];
        void run(int k) { store_piece(dst + lo[k], src + lo[k], lo[k + 1] - lo[k]); done.fetch_add(1, std::memory_order_release); }
    };
    auto sp = std::make_shared<Split>();
    const int pieces = helpers + 1;
    sp->dst = dst; sp->src = src;
    for (int k = 0; k <= pieces; ++k) sp->lo[k] = k == pieces ? n : (n * (size_t)k / (size_t)pieces) & ~(size_t)127;
    for (int k = 0; k < 3; ++k) sp->claimed[k].store(0, std::memory_order_relaxed);
    sp->claimed[0].store(1, std::memory_order_relaxed);
    for (int k = 1; k < pieces; ++k)
        if (host_submit_fn(0, [sp, k] { if (!sp->claimed[k].exchange(1, std::memory_order_acq_rel)) sp->run(k); }, false) != 0) break;   // (not submitted: claimed below)
    sp->run(0);
    for (int k = 1; k < pieces; ++k)
        if (!sp->claimed[k].exchange(1, std::memory_order_acq_rel)) sp->run(k);
    // (a helper that has claimed a piece finishes it in microseconds -- unless the scheduler has taken its core: then give ours up too)
    for (unsigned spins = 0; sp->done.load(std::memory_order_acquire) < pieces; ++spins) {
        if ((spins & 0xffffu) == 0xffffu) std::this_thread::yield(); else __builtin_ia32_pause();
    }
}
// Does the host KNOW that no kernel reads the camera rows of slots [first, first + n) any more?  Asked without a call that could
// cost the frame anything: hipStreamQuery on a stream whose last kernel carries no signal makes the runtime enqueue a marker and
// wait for it (measured: process() 172 -> 198 us per frame with two such queries in front of the stores) -- so the answer comes
// from what the library has seen itself: the recorded readers' events (a query of an existing signal), and for the unrecorded
// ones of a one-frame context the completion word the host polled at the end of the previous frame (RangeEvents::lazy_seen).
// "Not known" is not "busy": the caller then takes the engine's stream-ordered copy, which needs no answer.
bool camera_rows_known_idle(lt_ctx* c, int first, int n) {
    const lt_ctx::RangeEvents& r = c->readers;
    if (r.overflow || r.lazy_seen != r.lazy_seq) return false;
    for (unsigned i = 0; i < r.count; ++i) {
        const lt_ctx::RangeEvents::Entry& w = r.e[(r.head + i) % (unsigned)r.e.size()];
        if (w.lo < first + n && w.hi > first && hipEventQuery(w.ev) != hipSuccess) { (void)hipGetLastError(); return false; }
    }
    return true;
}

int Ingest::note_enqueued(hipStream_t st, int f0, int m) const {
    switch (kind) {
    case STAGED:        // the conversion that a rest puts on the copy stream reads the rows this copy brings into staging
        return note_range(c->yuv_rows, st, f0, f0 + m);
    case RESIZED: {     // the resize just launched reads staging (the next upload into it waits), and a rest's resize on the copy stream reads rows this copy brings
        const int rc = note_range_frame(c, c->readers, st, f0, f0 + m);
        return rc ? rc : note_range_frame(c, c->yuv_rows, st, f0, f0 + m);
    }
    default:            // where a later small call could take the aperture, this copy counts as work on the slots' rows that the host has not seen
                        // finished: stores from the host must not be overtaken by it
        if (c->direct_upload == 1 && (size_t)m * (size_t)(path.r1 - path.r0) * (size_t)c->calib.img_w * 3 <= APERTURE_MAX_BYTES)
            return note_range_frame(c, c->readers, st, f0, f0 + m);
        return LT_OK;
    }
}

// ---- the rows the path reads: lt_upload_frame_rows, _enqueue, _async ---------------------------------------------------------------
// One body; what varies is where the copy goes and who waits:
//   WAITED        the context stream, behind a wait for the whole context, and the host waits for the copy
//   SLOT_STREAMS  the slots' own streams (behind everything launched over these slots there, ahead of the kernels lt_mask_run puts there)
//                 and behind the kernels of OTHER streams that still read the slots' camera rows -- overlays on the presentation stream
//                 (slot-range events); nobody waits.  From the caller's pageable frame the call returns once the runtime has the bytes on
//                 their way (22-27 us for one 1280x720 frame's rows against 49-54 with the wait: the engine's 18 us run under the mask
//                 chain's launches).  LT_UPLOAD_SYNC=1: wait for the whole context first, as WAITED does (A/B; 5-10 us of a process() frame,
//                 on its critical path)
//   COPY_STREAM   the copy stream, behind the kernels that still read these slots' camera rows (the undistortion launches over these
//                 slots, the overlay) -- not the rest of their mask chains, not launches over other slots; the slots' streams wait for it
//                 before anything enqueued later, so the upload of one slot range overlaps the chain of every other slot range
enum class RowsVia { WAITED, SLOT_STREAMS, COPY_STREAM };

int upload_rows(lt_ctx* c, const uint8_t* frames, int first, int n, RowsVia via) {
    int rc = check_upload(c, frames, first, n);
    if (rc || n == 0 || c->cam_r1 <= c->cam_r0) return rc;
    static const bool enqueue_syncs = [] { const char* e = LT_EXP_ENV("LT_UPLOAD_SYNC"); return e && e[0] == '1'; }();
    const bool synced = via == RowsVia::WAITED || (via == RowsVia::SLOT_STREAMS && enqueue_syncs);
    if (synced && (rc = sync_all(c))) return rc;
    mark_frames(c, first, n, 0);         // a new frame's rows: the others are the previous occupant's until lt_upload_frame_rest
    front_stale(c, first, n);
    const Ingest in = ingest_of(c);
    // the path's rows of frames f0 - first ... into slots [f0, f0 + m), and -- unless the front end reads staging itself -- those rows of
    // the camera frames right behind them on the same stream
    auto put = [&](hipStream_t st, int f0, int m) {
        const int prc = in.copy(frames + (size_t)(f0 - first) * in.frame_pitch, f0, m, in.path, st);
        return prc || in.front_reads_staging ? prc : in.finish(st, f0, m, c->cam_r0, c->cam_r1);
    };
    switch (via) {
    case RowsVia::WAITED:
        if ((rc = put(c->stream, first, n))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        return LT_OK;
    case RowsVia::SLOT_STREAMS: {
        const size_t row_bytes = (size_t)c->calib.img_w * 3, off = (size_t)in.path.r0 * row_bytes, bytes = (size_t)(in.path.r1 - in.path.r0) * row_bytes;
        if (in.kind == Ingest::DIRECT && !enqueue_syncs && (size_t)n * bytes <= APERTURE_MAX_BYTES && direct_upload_possible(c) && camera_rows_known_idle(c, first, n)) {
            // a frame or two, and nothing left on the device that reads these slots' rows: by this thread's own stores (above); the
            // caller's array is free again when the call returns
            for (int k = 0; k < n; ++k)
                store_through_aperture(slot_frame(c, first + k) + off, frames + (size_t)k * c->frame_bytes + off, bytes);
            ++c->direct_uploads;
            return LT_OK;
        }
        return for_each_slice(c, first, n, [&](hipStream_t st, int f0, int m) {
            int wrc = enqueue_syncs ? (int)LT_OK : wait_camera_readers(c, st, f0, m);
            if (!wrc) wrc = put(st, f0, m);
            return wrc ? wrc : in.note_enqueued(st, f0, m);
        });
    }
    default: {
        if ((rc = wait_camera_readers(c, c->copy, first, n))) return rc;
        if ((rc = put(c->copy, first, n))) return rc;
        hipEvent_t up = next_order_event(c);
        if (!up) return fail(LT_ERR_HIP, "hipEventCreate failed");
        HIP_TRY(hipEventRecord(up, c->copy));
        return for_each_slice(c, first, n, [&](hipStream_t st, int, int) {
            HIP_TRY(hipStreamWaitEvent(st, up, 0));
            return (int)LT_OK;
        });
    }
    }
}

// ---- the rows a shown frame needs: lt_upload_frame_rest, _rest_rows, lt_device_frames_rest -----------------------------------------
// the copy stream waits for the enqueued uploads of the path's rows into the staging frames of slots [first, first + n) (the
// synchronous form has finished, the stream-ordered one is on the copy stream itself)
int wait_yuv_rows(lt_ctx* c, int first, int n) {
    bool precise = true;
    int rc = wait_range(c->yuv_rows, c->copy, first, first + n, &precise);
    if (!rc && !precise) rc = wait_reader_tails(c, c->copy);
    return rc;
}
// the overlay (on the presentation stream) waits for the copies into its own slots before it reads the frames (or, when the
// ring of slot ranges has overflowed, for the most recent copy)
int rest_mark(lt_ctx* c, int first, int n) {
    if (!c->rest_done && hipEventCreateWithFlags(&c->rest_done, hipEventDisableTiming) != hipSuccess) return fail(LT_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(c->rest_done, c->copy));
    c->rest_pending = true;
    return note_range(c->rests, c->copy, first, first + n);
}
// The two runs of rows of a rest: rows4, checked, or -- null -- the whole frame as the runs {0, H, H, H}.
struct Runs { int32_t r[4]; };
int rest_runs(const lt_ctx* c, const int32_t* rows4, Runs* out) {
    const int H = c->calib.img_h;
    if (rows4 && !(0 <= rows4[0] && rows4[0] <= rows4[1] && rows4[1] <= rows4[2] && rows4[2] <= rows4[3] && rows4[3] <= H))
        return fail(LT_ERR_INVALID, "row runs must be ordered and inside the frame");
    *out = rows4 ? Runs{{rows4[0], rows4[1], rows4[2], rows4[3]}} : Runs{{0, H, H, H}};
    return LT_OK;
}

// On the copy stream beside the compute streams.  These rows are read by nobody but the overlay: the copy waits for the overlays still
// reading the frames it replaces (slot-range events; a stream of windows re-uses its slots), and the overlay of these slots waits for it.
int upload_rest(lt_ctx* c, const uint8_t* frames, int first, int n, const int32_t* rows4) {
    int rc = check_upload(c, frames, first, n);
    if (rc) return rc;
    Runs runs;
    if ((rc = rest_runs(c, rows4, &runs)) || n == 0) return rc;
    if ((rc = wait_camera_readers(c, c->copy, first, n))) return rc;
    const Ingest in = ingest_of(c);
    // of the two runs, the camera rows the path's upload has not made: below the window of rows the path reads, and above it (staged: it
    // made none -- both runs whole, the path's rows they cover included, which that upload left in staging)
    int pieces[4][2], np = 0;
    for (int k = 0; k < 4; k += 2) {
        const int piece[2][2] = {{runs.r[k], std::min(runs.r[k + 1], in.made0)}, {std::max(runs.r[k], in.made1), runs.r[k + 1]}};
        for (const auto& pc : piece)
            if (pc[1] > pc[0]) { pieces[np][0] = pc[0]; pieces[np][1] = pc[1]; ++np; }
    }
    for (int i = 0; i < np; ++i)
        if ((rc = in.copy_rest(frames, first, n, pieces[i][0], pieces[i][1], c->copy))) return rc;
    if (in.staging) {
        // behind the enqueued uploads of the path's rows (the finish reads them, or rows next to them), the pieces' finish
        if ((rc = wait_yuv_rows(c, first, n))) return rc;
        for (int i = 0; i < np; ++i)
            if ((rc = in.finish(c->copy, first, n, pieces[i][0], pieces[i][1]))) return rc;
        if ((rc = note_range(c->readers, c->copy, first, first + n))) return rc;     // the finish reads staging: the next upload into it waits
    }
    if (!rows4) mark_frames(c, first, n, 1);
    return rest_mark(c, first, n);
}

// the pointer-list forms: frames[k] into slot first + k by the one-frame form, once the whole list is checked
int upload_list(lt_ctx* c, const uint8_t* const* frames, int first, int n, const char* what,
                int (*one)(lt_ctx*, const uint8_t*, int, int)) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (n > 0 && !frames) return fail(LT_ERR_INVALID, "null frame list");
    for (int k = 0; k < n; ++k)
        if (!frames[k]) return fail(LT_ERR_INVALID, "%s: frame %d is null", what, k);
    for (int k = 0; k < n; ++k)
        if ((rc = one(c, frames[k], first + k, 1))) return rc;
    return LT_OK;
}

}  // namespace

extern "C" {

int lt_get_input_rows(lt_ctx* c, int* row0, int* row1) {
    if (!c || !row0 || !row1) return fail(LT_ERR_INVALID, "null argument");
    const Rows r = ingest_of(c).rows_for(c->cam_r0, c->cam_r1, false);
    *row0 = r.r0;
    *row1 = r.r1;
    return LT_OK;
}

int lt_set_direct_upload(lt_ctx* c, int on) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (on >= 0) c->direct_upload_wanted = on != 0;
    return direct_upload_possible(c) ? 1 : 0;
}
unsigned long long lt_direct_upload_count(lt_ctx* c) { return c ? c->direct_uploads : 0; }

// The whole frames, and the host waits: everything copied, the whole camera frame finished.
int lt_upload_frames(lt_ctx* c, const uint8_t* frames, int first, int n) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (!frames) return fail(LT_ERR_INVALID, "null frames");
    if ((rc = set_device(c))) return rc;
    if ((rc = sync_all(c))) return rc;
    if (n > 0) c->input_locked = true;
    detach_slots(c, first, n);
    const Ingest in = ingest_of(c);
    const int H = c->calib.img_h;
    if (n > 0 && (rc = in.copy(frames, first, n, in.rows_for(0, H, true), c->stream))) return rc;
    if (n > 0 && (rc = in.finish(c->stream, first, n, 0, H))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    mark_frames(c, first, n, 1);
    front_stale(c, first, n);
    return LT_OK;
}

int lt_upload_frame_rows(lt_ctx* c, const uint8_t* frames, int first, int n) { return upload_rows(c, frames, first, n, RowsVia::WAITED); }
int lt_upload_frame_rows_enqueue(lt_ctx* c, const uint8_t* frames, int first, int n) { return upload_rows(c, frames, first, n, RowsVia::SLOT_STREAMS); }
int lt_upload_frame_rows_async(lt_ctx* c, const uint8_t* frames, int first, int n) { return upload_rows(c, frames, first, n, RowsVia::COPY_STREAM); }

int lt_upload_frame_rest_rows(lt_ctx* c, const uint8_t* frames, int first, int n, const int32_t* rows4) { return upload_rest(c, frames, first, n, rows4); }
int lt_upload_frame_rest(lt_ctx* c, const uint8_t* frames, int first, int n) { return upload_rest(c, frames, first, n, nullptr); }

int lt_upload_frame_rows_list(lt_ctx* c, const uint8_t* const* frames, int first, int n) {
    return upload_list(c, frames, first, n, "lt_upload_frame_rows_list", lt_upload_frame_rows_enqueue);
}
int lt_upload_frame_rest_list(lt_ctx* c, const uint8_t* const* frames, int first, int n) {
    return upload_list(c, frames, first, n, "lt_upload_frame_rest_list", lt_upload_frame_rest);
}

// Frames that are already in device memory (lt_attach_device_frames): the rest's runs from the attached surfaces.
int lt_device_frames_rest(lt_ctx* c, int first, int n, const int32_t* rows4) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    for (int i = first; i < first + n; ++i)
        if (i >= (int)c->attached.size() || !c->attached[(size_t)i])
            return fail(LT_ERR_STATE, i < (int)c->drawn.size() && c->drawn[(size_t)i] ? "slot %d: its surface was drawn into in place (lt_overlay_run_inplace) and holds no camera frame any more"
                                                                                      : "slot %d has no device frame attached", i);
    Runs runs;
    if ((rc = rest_runs(c, rows4, &runs)) || n == 0) return rc;
    if ((rc = set_device(c))) return rc;
    // as lt_upload_frame_rest: on the copy stream, behind the overlays that still read the camera frames these rows replace
    if ((rc = wait_camera_readers(c, c->copy, first, n))) return rc;
    if ((rc = raw_sets_ready(c))) return rc;
    const RawRun raw = raw_run_of(c, first, n);
    for (int k = 0; k < 4; k += 2)
        launch_surf_rows_to_rgb(c->copy, c->in_layout, &c->surf[(size_t)first], yuv_coef_of(c), slot_frame(c, first), c->frame_bytes,
                                c->calib.img_h, c->calib.img_w, runs.r[k], runs.r[k + 1], n, raw.one, raw.sets, raw.ids);
    HIP_TRY(hipGetLastError());
    if ((rc = note_range(c->readers, c->copy, first, first + n))) return rc;      // it reads the surfaces and writes the camera frames: the next upload waits
    if (!rows4) mark_frames(c, first, n, 1);
    return rest_mark(c, first, n);
}

}  // extern "C"
