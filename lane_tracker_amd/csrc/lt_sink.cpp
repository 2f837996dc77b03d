// Device sinks of liblane_tracker_amd.so: dense RGB frames of the library -- the annotated frames of a context, or any block of
// lt_device_alloc -- written into surfaces the caller owns, RGB, BGR, RGBA, BGRA, NV12 or I420 at the caller's pitches (k_sink.hip).  The way out
// that mirrors lt_attach_device_frames: a pipeline of decoder, lane tracker and encoder never crosses the bus with a frame.
// Everything is checked on the host before anything is launched; a refused call leaves the context as it was.
#include <algorithm>
#include <cstring>
#include <vector>

#include "lt_ctx.h"
#include "sink_arith.h"

using namespace lt;

namespace {

struct ByteRange { uintptr_t lo, hi; int surface, plane; };   // [lo, hi)

// (rows, row bytes) of plane i of an h x w frame in `layout`
inline void plane_geom(int layout, int h, int w, int i, int* rows, int* row_bytes) {
    if (i == 0) { *rows = h; *row_bytes = one_plane_row_bytes(layout, w) ? one_plane_row_bytes(layout, w) : w; }   // (4:2:2, raw Bayer: an attached camera surface only)
    else { *rows = h / 2; *row_bytes = layout == LT_INPUT_NV12 ? w : w / 2; }
}
inline int plane_count(int layout) { return one_plane_row_bytes(layout, 4) ? 1 : layout + 1; }

int check_format(int layout, int h, int w, const int32_t* coeffs) {
    if (layout != LT_INPUT_RGB && layout != LT_INPUT_NV12 && layout != LT_INPUT_I420 && !is_rgb_family(layout))
        return fail(LT_ERR_INVALID, "sink layout must be RGB (0), NV12 (1), I420 (2), BGR (5), RGBA (6) or BGRA (7): packed 4:2:2 is an input format only, and so is raw Bayer");
    if (h < 1 || w < 1 || h > 16384 || w > 16384) return fail(LT_ERR_INVALID, "bad image size %dx%d (at most 16384 x 16384)", w, h);
    if (layout == LT_INPUT_RGB || is_rgb_family(layout)) return LT_OK;
    if ((h & 1) || (w & 1)) return fail(LT_ERR_INVALID, "4:2:0 surfaces need an even width and height, got %dx%d", w, h);
    if (!coeffs) return fail(LT_ERR_INVALID, "a 4:2:0 sink needs its eight conversion coefficients");
    if (!sa::coeffs_ok(coeffs))
        return fail(LT_ERR_INVALID, "conversion coefficients must be below 2^23 in magnitude and keep every row's sum inside 32 bits");
    return LT_OK;
}

// Every plane of every destination through check_plane's rules; no two planes of the call may share a byte.  -> the kernels'
// entries and the planes' byte ranges, sorted.
int check_sinks(int device, const lt_device_surface* dst, int n, int layout, int h, int w, std::vector<SurfEntry>& ent,
                std::vector<ByteRange>& ranges) {
    constexpr int PITCH_MAX = (1 << 23) - 1;
    const int planes = plane_count(layout);
    KnownRange memo;
    ent.assign((size_t)n, SurfEntry{});
    ranges.clear();
    ranges.reserve((size_t)n * planes);
    for (int k = 0; k < n; ++k) {
        const lt_device_surface& f = dst[k];
        for (int i = 0; i < planes; ++i) {
            int rows, rb;
            plane_geom(layout, h, w, i, &rows, &rb);
            const int pitch = i == 0 ? f.pitch : f.chroma_pitch;
            if (pitch < rb) return fail(LT_ERR_INVALID, "surface %d: %spitch %d is below the row's %d bytes", k, i ? "chroma " : "", pitch, rb);
            if (pitch > PITCH_MAX) return fail(LT_ERR_INVALID, "surface %d: %spitch %d is too large", k, i ? "chroma " : "", pitch);
            const size_t ext = (size_t)pitch * (size_t)(rows - 1) + (size_t)rb;
            const int rc = check_plane(device, f.plane[i], ext, k, i, memo);
            if (rc) return rc;
            ent[(size_t)k].plane[i] = (uint64_t)(uintptr_t)f.plane[i];
            ranges.push_back(ByteRange{(uintptr_t)f.plane[i], (uintptr_t)f.plane[i] + ext, k, i});
        }
        ent[(size_t)k].pitch = f.pitch;
        ent[(size_t)k].cpitch = planes == 1 ? 0 : f.chroma_pitch;
    }
    std::sort(ranges.begin(), ranges.end(), [](const ByteRange& a, const ByteRange& b) { return a.lo < b.lo; });
    for (size_t j = 1; j < ranges.size(); ++j)
        if (ranges[j].lo < ranges[j - 1].hi)
            return fail(LT_ERR_INVALID, "surface %d plane %d overlaps surface %d plane %d: the destinations of one call must be disjoint",
                        ranges[j].surface, ranges[j].plane, ranges[j - 1].surface, ranges[j - 1].plane);
    return LT_OK;
}

// the first of the sorted, disjoint `ranges` that shares a byte with [lo, hi), or null
const ByteRange* overlapping(const std::vector<ByteRange>& ranges, uintptr_t lo, uintptr_t hi) {
    auto it = std::upper_bound(ranges.begin(), ranges.end(), lo, [](uintptr_t v, const ByteRange& r) { return v < r.hi; });   // first with hi > lo
    return it != ranges.end() && it->lo < hi ? &*it : nullptr;
}

}  // namespace

namespace lt {

// (the one-launch draw of lt_overlay_run_to_surfaces, k_draw_sink.hip: RGB, NV12 and I420 only)
int check_sink_format(int layout, int h, int w, const int32_t* coeffs) {
    if (is_rgb_family(layout)) return fail(LT_ERR_INVALID, "lt_overlay_run_to_surfaces draws into RGB (0), NV12 (1) or I420 (2) surfaces: BGR / RGBA / BGRA sinks take lt_overlay_store_device");
    return check_format(layout, h, w, coeffs);
}

int check_ctx_sinks(lt_ctx* c, const lt_device_surface* dst, int n, int layout, std::vector<SurfEntry>& ent) {
    const int H = c->calib.img_h, W = c->calib.img_w;
    std::vector<ByteRange> ranges;
    int rc = check_sinks(c->device, dst, n, layout, H, W, ent, ranges);
    if (rc) return rc;
    // The front end of an attached slot reads its surface whenever its next lt_mask_run / lt_device_frames_rest comes: a sink
    // may not share a byte with any of them (the host mirror of the surface table says where they are).
    const int in_planes = plane_count(c->in_layout);
    for (size_t s = 0; s < c->attached.size(); ++s) {
        if (!c->attached[s]) continue;
        const SurfEntry& a = c->surf[s];
        for (int i = 0; i < in_planes; ++i) {
            int rows, rb;
            plane_geom(c->in_layout, H, W, i, &rows, &rb);
            const uintptr_t lo = (uintptr_t)a.plane[i], hi = lo + (size_t)(i == 0 ? a.pitch : a.cpitch) * (size_t)(rows - 1) + (size_t)rb;
            if (const ByteRange* r = overlapping(ranges, lo, hi))
                return fail(LT_ERR_INVALID, "surface %d plane %d overlaps the camera surface attached to slot %d: annotating a surface in place is not supported",
                            r->surface, r->plane, (int)s);
        }
    }
    return LT_OK;
}

}  // namespace lt

extern "C" {

int lt_rgb_to_surfaces(int device, const void* rgb, size_t frame_stride, int h, int w, int n, const lt_device_surface* dst, int layout,
                       const int32_t* coeffs) {
    if (n < 0) return fail(LT_ERR_INVALID, "negative frame count");
    int rc = check_format(layout, h, w, coeffs);
    if (rc) return rc;
    if (n == 0) return LT_OK;
    if (!rgb || !dst) return fail(LT_ERR_INVALID, "null argument");
    const size_t frame = (size_t)h * w * 3;
    if (frame_stride < frame) return fail(LT_ERR_INVALID, "frame stride %zu is below a frame's %zu bytes", frame_stride, frame);
    const void* base = nullptr;
    size_t size = 0;
    int dev = 0;
    const size_t src_ext = frame_stride * (size_t)(n - 1) + frame;
    if (!cached_block_find(rgb, &base, &size, &dev) || (uintptr_t)rgb + src_ext > (uintptr_t)base + size)
        return fail(LT_ERR_INVALID, "lt_rgb_to_surfaces: %zu bytes of RGB frames at %p do not lie inside a block of lt_device_alloc", src_ext, rgb);
    if (dev != device) return fail(LT_ERR_INVALID, "lt_rgb_to_surfaces: the RGB frames lie on device %d, not on device %d", dev, device);
    std::vector<SurfEntry> ent;
    std::vector<ByteRange> ranges;
    if ((rc = check_sinks(device, dst, n, layout, h, w, ent, ranges))) return rc;
    if (const ByteRange* r = overlapping(ranges, (uintptr_t)rgb, (uintptr_t)rgb + src_ext))
        return fail(LT_ERR_INVALID, "surface %d plane %d overlaps the RGB frames it is written from", r->surface, r->plane);
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != device) HIP_TRY(hipSetDevice(device));
    hipStream_t st = nullptr;
    hipError_t e = stream_get(&st, SK_PLAIN, 0);
    if (e == hipSuccess) {
        launch_rgb_to_surfaces(st, layout, static_cast<const uint8_t*>(rgb), frame_stride, h, w, ent.data(), n, coeffs);
        e = hipGetLastError();
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
        stream_put(st);
    }
    if (cur != device) (void)hipSetDevice(cur);
    if (e != hipSuccess) return fail(LT_ERR_HIP, "lt_rgb_to_surfaces failed: %s", hipGetErrorString(e));
    return LT_OK;
}

int lt_overlay_store_device(lt_ctx* c, int first, int n, const lt_device_surface* dst, int layout, const int32_t* coeffs) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    const int H = c->calib.img_h, W = c->calib.img_w;
    if ((rc = check_format(layout, H, W, coeffs))) return rc;
    if (n == 0) return LT_OK;
    if (!dst) return fail(LT_ERR_INVALID, "null surfaces");
    if (!c->d_annot || !c->present) return fail(LT_ERR_STATE, "lt_overlay_store_device before lt_overlay_run");
    {
        const int bad = first_partial(c->annot_full, first, n);
        if (bad >= 0) return fail(LT_ERR_STATE, "slot %d holds row runs of its annotated frame only (lt_overlay_run_rows / lt_present_*): no whole frame to store", bad);
    }
    if ((rc = set_device(c))) return rc;
    std::vector<SurfEntry> ent;
    if ((rc = check_ctx_sinks(c, dst, n, layout, ent))) return rc;
    if (!c->store_done && hipEventCreateWithFlags(&c->store_done, hipEventDisableTiming) != hipSuccess) return fail(LT_ERR_HIP, "hipEventCreate failed");
    // On the presentation stream: behind the lt_overlay_run / lt_overlay_text that wrote these frames, ahead of the next ones over
    // the same slots.  The store only reads the annotated frames, so a download in flight on the download stream is no hazard.
    launch_rgb_to_surfaces(c->present, layout, c->d_annot + (size_t)first * c->frame_bytes, c->frame_bytes, H, W, ent.data(), n, coeffs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->store_done, c->present));
    c->store_pending = true;
    return LT_OK;
}

int lt_overlay_store_wait(lt_ctx* c) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (!c->store_pending) return LT_OK;
    int rc = set_device(c);
    if (rc) return rc;
    HIP_TRY(hipEventSynchronize(c->store_done));
    c->store_pending = false;
    return LT_OK;
}

}  // extern "C"
