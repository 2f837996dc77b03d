// Search visualisations and split-view panes of listed frames (lane_tracker.py:687-793, 1130-1137) from what the slots hold, and
// the single-image cv2.resize(INTER_LINEAR): lt_search_viz_run, lt_split_panes_run, lt_split_panes_size, lt_search_viz_wait,
// lt_resize_linear_u8.  The host's share: the band polygons' row intervals (lt_lane_polygon_spans, as overlay.fill_band), the plot
// points as they come, the resize taps (utils._resize_taps) and the ordering; the kernels are in k_search_viz.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "lt_ctx.h"

namespace lt {

// cv2.resize INTER_LINEAR along one axis, in the operations of utils._resize_taps: per destination index (tap 0, tap 1, coefficient 0,
// coefficient 1)
static void resize_taps(int src_len, int dst_len, std::vector<int32_t>& t) {
    t.resize((size_t)4 * dst_len);
    const double scale = (double)src_len / (double)dst_len;
    for (int i = 0; i < dst_len; ++i) {
        float f = (float)(((double)i + 0.5) * scale - 0.5);
        const float fl = std::floor(f);
        long long s = (long long)fl;
        f = f - fl;
        if (s < 0) { s = 0; f = 0.f; }
        else if (s >= src_len - 1) { s = src_len - 1; f = 0.f; }
        const float c1 = std::nearbyint(f * 2048.f), c0 = std::nearbyint((1.f - f) * 2048.f);
        t[4 * (size_t)i] = (int32_t)s;
        t[4 * (size_t)i + 1] = (int32_t)std::min<long long>(s + 1, src_len - 1);
        t[4 * (size_t)i + 2] = (int32_t)c0;
        t[4 * (size_t)i + 3] = (int32_t)c1;
    }
}

// triple_split_view's size arithmetic (lane_tracker.py:781-787): Python's round() is round-half-even, as nearbyint
static void panes_size(const lt_calib& k, int* sw, int* sh, int* x2) {
    const double half = 0.5 * k.img_w, scale = k.warp_w / half;
    *x2 = (int)std::nearbyint(half);
    *sw = (int)std::nearbyint(k.warp_w / scale);
    *sh = (int)std::nearbyint(k.warp_h / scale);
}

void viz_free_device(lt_ctx* c) {
    VizRing& r = c->viz;
    dev_free(r.d_pics);
    dev_free(r.d_bev);
    dev_free(r.d_panes);
    dev_free(r.d_xt);
    dev_free(r.d_yt);
    for (auto& h : r.half) {
        dev_free(h.d_stage);
        h.d_bytes = 0;
    }
}

void viz_free_host(lt_ctx* c) {
    VizRing& r = c->viz;
    for (auto& h : r.half) {
        if (h.staged) (void)hipEventDestroy(h.staged);
        if (h.copied) (void)hipEventDestroy(h.copied);
        if (h.h_stage) (void)hipHostFree(h.h_stage);
        h.staged = h.copied = nullptr;
        h.staged_set = h.copied_set = false;
        h.h_stage = nullptr;
        h.h_bytes = 0;
    }
    r.last = nullptr;
}

static int ensure_ring(lt_ctx* c, bool panes) {
    VizRing& r = c->viz;
    const lt_calib& k = c->calib;
    int rc;
    if (!r.d_pics && (rc = dev_alloc(&r.d_pics, (size_t)VizRing::FRAMES * c->bev_bytes))) return rc;
    for (auto& h : r.half) {
        if (!h.staged && hipEventCreateWithFlags(&h.staged, hipEventDisableTiming) != hipSuccess) return fail(LT_ERR_HIP, "hipEventCreate failed");
        if (!h.copied && hipEventCreateWithFlags(&h.copied, hipEventDisableTiming) != hipSuccess) return fail(LT_ERR_HIP, "hipEventCreate failed");
    }
    if (!c->present && create_compute_stream(&c->present, c->search_cus) != hipSuccess) return fail(LT_ERR_HIP, "hipStreamCreate failed");
    if (!c->dl) HIP_TRY(stream_get(&c->dl, SK_PRIORITY, 0));
    if (!panes) return LT_OK;
    int sw, sh, x2;
    panes_size(k, &sw, &sh, &x2);
    if (sw < 1 || sh < 1) return fail(LT_ERR_STATE, "split view: the scaled bird's-eye image is empty");
    if (!r.d_bev && (rc = dev_alloc(&r.d_bev, (size_t)VizRing::FRAMES * c->bev_bytes))) return rc;
    if (!r.d_panes && (rc = dev_alloc(&r.d_panes, (size_t)VizRing::FRAMES * sh * k.img_w * 3))) return rc;
    if (!r.d_xt) {
        std::vector<int32_t> xt, yt;
        resize_taps(k.warp_w, sw, xt);
        resize_taps(k.warp_h, sh, yt);
        if ((rc = dev_alloc(&r.d_xt, xt.size())) || (rc = dev_alloc(&r.d_yt, yt.size()))) return rc;
        HIP_TRY(hipMemcpy(r.d_xt, xt.data(), xt.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(r.d_yt, yt.data(), yt.size() * 4, hipMemcpyHostToDevice));
    }
    return LT_OK;
}

int warm_search_viz(lt_ctx* c, bool panes) { return ensure_ring(c, panes); }

// one side's band polygon as overlay.fill_band forms it -- (x - bandwidth, y) ... then the reversed (x + bandwidth, y) -- as row
// intervals clipped to the image; a row the polygon does not touch is (1, 0)
static void band_spans(int h, int w, const int32_t* yx, int n, int bandwidth, std::vector<int32_t>& lo, std::vector<int32_t>& hi, int16_t* out) {
    lo.resize((size_t)2 * std::max(n, 1));
    hi.resize((size_t)2 * std::max(n, 1));
    for (int i = 0; i < n; ++i) {
        lo[2 * (size_t)i] = hi[2 * (size_t)i] = yx[2 * i];
        lo[2 * (size_t)i + 1] = yx[2 * i + 1] - bandwidth;
        hi[2 * (size_t)i + 1] = yx[2 * i + 1] + bandwidth;
    }
    (void)lt_lane_polygon_spans(h, lo.data(), n, hi.data(), n, out);
    for (int y = 0; y < h; ++y) {
        int a = out[2 * y], b = out[2 * y + 1];
        if (a <= b) { a = std::max(a, 0); b = std::min(b, w - 1); }
        if (a > b) { a = 1; b = 0; }
        out[2 * y] = (int16_t)a;
        out[2 * y + 1] = (int16_t)b;
    }
}

static int viz_run(lt_ctx* c, int n, const lt_viz_item* items, const int32_t* fl, const int32_t* fr, const int32_t* bl, const int32_t* br,
                   uint8_t* out_host, bool panes, const char* who) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (n < 0 || (n > 0 && (!items || !out_host))) return fail(LT_ERR_INVALID, "%s: n < 0, a null item list or a null output", who);
    long long tfl = 0, tfr = 0, tbl = 0, tbr = 0;
    bool lists = false, windows = false;
    for (int i = 0; i < n; ++i) {
        const lt_viz_item& it = items[i];
        if (it.slot < 0 || it.slot >= c->capacity) return fail(LT_ERR_INVALID, "%s: item %d: slot %d outside capacity %d", who, i, it.slot, c->capacity);
        if (it.kind < 0 || it.kind > 2) return fail(LT_ERR_INVALID, "%s: item %d: kind %d (0 mask, 1 sliding window, 2 band)", who, i, it.kind);
        if (it.n_fit_left < 0 || it.n_fit_right < 0 || it.n_band_left < 0 || it.n_band_right < 0)
            return fail(LT_ERR_INVALID, "%s: item %d: negative point count", who, i);
        if (it.kind == 1 && it.window_height <= 0) return fail(LT_ERR_INVALID, "%s: item %d: window_height must be positive", who, i);
        if (it.kind != 0) { tfl += it.n_fit_left; tfr += it.n_fit_right; lists = true; }
        if (it.kind == 1) windows = true;
        if (it.kind == 2) { tbl += it.n_band_left; tbr += it.n_band_right; }
    }
    if ((tfl && !fl) || (tfr && !fr) || (tbl && !bl) || (tbr && !br)) return fail(LT_ERR_INVALID, "%s: a point list the items need is null", who);
    if (n == 0) return LT_OK;
    for (int i = 0; i < n; ++i) {        // (the bird's-eye images of the split view are warped with the context's own table)
        const int rrc = refuse_foreign(c, items[i].slot, 1, who);
        if (rrc) return rrc;
    }
    if (!c->have_mask) return fail(LT_ERR_STATE, "%s: no mask in the slots: run lt_mask_run or lt_upload_masks first", who);
    for (int i = 0; i < n; ++i)
        if (!c->mask_bits_ok[(size_t)items[i].slot] && !c->masks.d_plane[P_MASK])
            return fail(LT_ERR_STATE, "%s: slot %d holds no mask", who, items[i].slot);
    if (lists && !c->d_pix) return fail(LT_ERR_STATE, "%s: no search has run yet", who);
    if (windows && !c->d_cent) return fail(LT_ERR_STATE, "%s: no sliding-window search has run yet", who);
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = ensure_ring(c, panes))) return rc;
    VizRing& ring = c->viz;
    const int h = c->calib.warp_h, w = c->calib.warp_w, img_w = c->calib.img_w;
    hipStream_t ps = c->present;

    // behind whatever wrote the listed slots (masks, searches, chains), run of consecutive slots by run
    std::vector<int> slots((size_t)n);
    for (int i = 0; i < n; ++i) slots[(size_t)i] = items[i].slot;
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    const int k = slice_count(c);
    std::vector<uint8_t> touched((size_t)k, 0);
    for (int s : slots) touched[(size_t)slice_of(c, s)] = 1;
    bool tails = false;
    for (size_t a = 0; a < slots.size();) {
        size_t b = a + 1;
        while (b < slots.size() && slots[b] == slots[b - 1] + 1) ++b;
        bool precise = true;
        if ((rc = wait_range(c->writers, ps, slots[a], slots[b - 1] + 1, &precise))) return rc;
        tails = tails || !precise;
        if ((rc = wait_chains(c, ps, slots[a], slots[b - 1] + 1))) return rc;
        a = b;
    }
    if (tails) {
        for (int si = 0; si < k; ++si)
            if (touched[(size_t)si] && (rc = wait_tail(c, ps, c->streams[(size_t)si]))) return rc;
        if (c->urgent && (rc = wait_tail(c, ps, c->urgent))) return rc;
    }

    int sw = 0, sh = 0, x2 = 0;
    if (panes) panes_size(c->calib, &sw, &sh, &x2);
    const size_t pic = c->bev_bytes, strip = (size_t)sh * img_w * 3, out_bytes = panes ? strip : pic;
    const size_t span_bytes = (size_t)2 * h * 2 * sizeof(int16_t);
    std::vector<int32_t> tmp_lo, tmp_hi;
    size_t ofl = 0, ofr = 0, obl = 0, obr = 0;          // points consumed from the four lists
    for (int at = 0; at < n; at += VizRing::HALF) {
        const int m = std::min(VizRing::HALF, n - at);
        const int hi_ = ring.next;
        VizRing::Half& half = ring.half[hi_];
        ring.next ^= 1;
        // the staging of this half: its last kernels have read it
        if (half.staged_set) HIP_TRY(hipEventSynchronize(half.staged));
        size_t need = 0;
        for (int i = 0; i < m; ++i) {
            const lt_viz_item& it = items[at + i];
            if (it.kind == 2) need += span_bytes;
            if (it.kind != 0) need += ((size_t)it.n_fit_left + it.n_fit_right) * 8;
        }
        need = (need + 15) & ~(size_t)15;
        if (need > half.h_bytes) {
            if (half.h_stage) (void)hipHostFree(half.h_stage);
            half.h_stage = nullptr;
            half.h_bytes = 0;
            const size_t cap = std::max(need, (size_t)VizRing::HALF * (span_bytes + (size_t)4 * h * 8));
            if (hipHostMalloc(reinterpret_cast<void**>(&half.h_stage), cap, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                half.h_stage = nullptr;
                return fail(LT_ERR_NOMEM, "hipHostMalloc(%zu) failed", cap);
            }
            half.h_bytes = cap;
        }
        if (need > half.d_bytes) {
            dev_free(half.d_stage);
            half.d_bytes = 0;
            if ((rc = dev_alloc(&half.d_stage, half.h_bytes))) return rc;
            half.d_bytes = half.h_bytes;
        }
        VizBatch batch;
        std::memset(&batch, 0, sizeof batch);
        size_t off = 0;
        for (int i = 0; i < m; ++i) {
            const lt_viz_item& it = items[at + i];
            VizFrame& f = batch.f[i];
            const int s = it.slot;
            if (c->mask_bits_ok[(size_t)s]) f.bits = c->masks.d_bits_open + (size_t)s * c->masks.bits_stride;
            else f.mask = slot_mask(c, s);
            f.rec = slot_rec(c, s);
            f.out = ring.d_pics + (size_t)(hi_ * VizRing::HALF + i) * pic;
            f.kind = it.kind;
            f.ww = it.window_width;
            f.wh = it.window_height;
            f.H1 = h - it.ignore_bottom;
            if (it.kind == 0) continue;
            f.pix = slot_pix(c, s);
            if (it.kind == 1) f.cent = slot_cent(c, s);
            if (it.kind == 2) {
                int16_t* sp = reinterpret_cast<int16_t*>(half.h_stage + off);
                band_spans(h, w, bl ? bl + 2 * obl : nullptr, it.n_band_left, it.bandwidth, tmp_lo, tmp_hi, sp);
                band_spans(h, w, br ? br + 2 * obr : nullptr, it.n_band_right, it.bandwidth, tmp_lo, tmp_hi, sp + (size_t)2 * h);
                f.band = reinterpret_cast<const int16_t*>(half.d_stage + off);
                off += span_bytes;
                obl += (size_t)it.n_band_left;
                obr += (size_t)it.n_band_right;
            }
            f.n_fit_left = it.n_fit_left;
            f.n_fit_right = it.n_fit_right;
            f.pts = reinterpret_cast<const int32_t*>(half.d_stage + off);
            if (it.n_fit_left) std::memcpy(half.h_stage + off, fl + 2 * ofl, (size_t)it.n_fit_left * 8);
            off += (size_t)it.n_fit_left * 8;
            if (it.n_fit_right) std::memcpy(half.h_stage + off, fr + 2 * ofr, (size_t)it.n_fit_right * 8);
            off += (size_t)it.n_fit_right * 8;
            ofl += (size_t)it.n_fit_left;
            ofr += (size_t)it.n_fit_right;
        }
        if (off) HIP_TRY(hipMemcpyAsync(half.d_stage, half.h_stage, off, hipMemcpyHostToDevice, ps));
        // the half's pictures of two pieces ago have left for the host
        if (half.copied_set) HIP_TRY(hipStreamWaitEvent(ps, half.copied, 0));
        launch_search_viz(ps, batch, m, h, w, (w + 63) / 64, c->maxpix, c->maxlev);
        const uint8_t* d_out = ring.d_pics + (size_t)hi_ * VizRing::HALF * pic;
        if (panes) {
            uint8_t* bev = ring.d_bev + (size_t)hi_ * VizRing::HALF * pic;
            uint8_t* dst = ring.d_panes + (size_t)hi_ * VizRing::HALF * strip;
            if (c->fe.nrows <= 0) HIP_TRY(hipMemsetAsync(bev, 0, (size_t)m * pic, ps));
            else
                for (int i = 0; i < m;) {          // the bird's-eye images, run of consecutive slots by run (k_warp_rgb, as lt_download_bev)
                    int j = i + 1;
                    while (j < m && items[at + j].slot == items[at + j - 1].slot + 1) ++j;
                    launch_warp_rgb(ps, c->d_und, c->und_px, items[at + i].slot, c->d_wxy, c->d_wfrac, c->fe, bev + (size_t)i * pic, pic, j - i);
                    i = j;
                }
            const int w1 = std::min(sw, img_w), w2 = std::max(0, std::min(sw, img_w - x2));
            if (w1 < x2 || x2 + w2 < img_w || w2 == 0) HIP_TRY(hipMemsetAsync(dst, 0, (size_t)m * strip, ps));   // bytes no pane covers
            launch_resize_linear_u8(ps, bev, pic, w, 3, dst, strip, img_w * 3, 0, w1, sh, ring.d_xt, ring.d_yt, m);
            launch_resize_linear_u8(ps, d_out, pic, w, 3, dst, strip, img_w * 3, x2, w2, sh, ring.d_xt, ring.d_yt, m);
            d_out = dst;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(half.staged, ps));
        half.staged_set = true;
        HIP_TRY(hipStreamWaitEvent(c->dl, half.staged, 0));
        HIP_TRY(hipMemcpyAsync(out_host + (size_t)at * out_bytes, d_out, (size_t)m * out_bytes, hipMemcpyDeviceToHost, c->dl));
        HIP_TRY(hipEventRecord(half.copied, c->dl));
        half.copied_set = true;
        ring.last = half.copied;
    }
    // later work over the listed slots -- a second try's mask, the next search, the region's next window -- behind the reads
    for (size_t a = 0; a < slots.size();) {
        size_t b = a + 1;
        while (b < slots.size() && slots[b] == slots[b - 1] + 1) ++b;
        if ((rc = note_written(c, ps, slots[a], slots[b - 1] + 1))) return rc;
        a = b;
    }
    hipEvent_t done = next_order_event(c);
    if (!done) return fail(LT_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(done, ps));
    for (int si = 0; si < k; ++si)
        if (touched[(size_t)si]) HIP_TRY(hipStreamWaitEvent(c->streams[(size_t)si], done, 0));
    return LT_OK;
}

}  // namespace lt

using namespace lt;

extern "C" {

int lt_search_viz_run(lt_ctx* c, int n, const lt_viz_item* items, const int32_t* fit_left_yx, const int32_t* fit_right_yx,
                      const int32_t* band_left_yx, const int32_t* band_right_yx, uint8_t* out_host) {
    return viz_run(c, n, items, fit_left_yx, fit_right_yx, band_left_yx, band_right_yx, out_host, false, "lt_search_viz_run");
}

int lt_split_panes_run(lt_ctx* c, int n, const lt_viz_item* items, const int32_t* fit_left_yx, const int32_t* fit_right_yx,
                       const int32_t* band_left_yx, const int32_t* band_right_yx, uint8_t* out_host) {
    return viz_run(c, n, items, fit_left_yx, fit_right_yx, band_left_yx, band_right_yx, out_host, true, "lt_split_panes_run");
}

int lt_calib_split_panes_size(const lt_calib* calib, int* scaled_w, int* scaled_h, int* second_x) {
    if (!calib || calib->img_w < 1 || calib->img_h < 1 || calib->warp_w < 1 || calib->warp_h < 1) return fail(LT_ERR_INVALID, "bad calibration sizes");
    int sw, sh, x2;
    panes_size(*calib, &sw, &sh, &x2);
    if (scaled_w) *scaled_w = sw;
    if (scaled_h) *scaled_h = sh;
    if (second_x) *second_x = x2;
    return LT_OK;
}

int lt_split_panes_size(lt_ctx* c, int* scaled_w, int* scaled_h, int* second_x) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    return lt_calib_split_panes_size(&c->calib, scaled_w, scaled_h, second_x);
}

int lt_search_viz_wait(lt_ctx* c) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (!c->viz.last) return LT_OK;
    int rc = set_device(c);
    if (rc) return rc;
    HIP_TRY(hipEventSynchronize(c->viz.last));
    c->viz.last = nullptr;
    return LT_OK;
}

int lt_resize_linear_u8(lt_ctx* c, const uint8_t* img, int h, int w, int channels, int dh, int dw, uint8_t* out) {
    if (!c || !img || !out) return fail(LT_ERR_INVALID, "null argument");
    if (h < 1 || w < 1 || dh < 1 || dw < 1 || h > 16384 || w > 16384 || dh > 16384 || dw > 16384) return fail(LT_ERR_INVALID, "bad image size");
    if (channels != 1 && channels != 3) return fail(LT_ERR_INVALID, "channels must be 1 or 3");
    int rc = set_device(c);
    if (rc) return rc;
    std::vector<int32_t> xt, yt;
    resize_taps(w, dw, xt);
    resize_taps(h, dh, yt);
    const size_t nin = (size_t)h * w * channels, nout = (size_t)dh * dw * channels;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    int32_t *d_xt = nullptr, *d_yt = nullptr;
    if ((rc = dev_alloc(&d_in, nin)) || (rc = dev_alloc(&d_out, nout)) || (rc = dev_alloc(&d_xt, xt.size())) || (rc = dev_alloc(&d_yt, yt.size()))) {
        dev_free(d_in); dev_free(d_out); dev_free(d_xt); dev_free(d_yt);
        return rc;
    }
    // (pageable sources: the copies are complete, as far as the host's buffers go, when the calls return)
    hipError_t e = hipMemcpyAsync(d_in, img, nin, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_xt, xt.data(), xt.size() * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_yt, yt.data(), yt.size() * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_resize_linear_u8(c->stream, d_in, nin, w, channels, d_out, nout, dw * channels, 0, dw, dh, d_xt, d_yt, 1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, nout, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(d_in); dev_free(d_out); dev_free(d_xt); dev_free(d_yt);
    if (e != hipSuccess) return fail(LT_ERR_HIP, "resize_linear_u8 failed: %s", hipGetErrorString(e));
    return LT_OK;
}

}  // extern "C"
