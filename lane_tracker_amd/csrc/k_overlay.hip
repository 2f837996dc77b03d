// Presentation stage on the device, gfx950.
//
//   k_overlay_lane   draw_lane()  lane_tracker.py:629-662 without the text:
//                    fillPoly((0,255,0)) on a blank bird's-eye image, warpPerspective(.., Minv, camera size),
//                    addWeighted(img, 1, lane, 0.3, 0)
//   k_warp_rgb       the bird's-eye RGB image itself (lane_tracker.py:1035) for split_view
//
// The filled polygon is never rasterised: it is y-monotone (both lane curves are functions of y), so
// it is described by one column interval [lo, hi] per bird's-eye row (built on the host from the
// 8-connected edge lines, lt_api.cpp).  The inverse warp is OpenCV's fixed-point bilinear remap of that
// 0/255 image: each camera pixel tests its four taps against the row intervals.  Only the green byte
// changes; 0.3*lane is added in f32 and rounded half-to-even like cv::addWeighted's saturate_cast.
#include <algorithm>
#include <cstring>
#include "lt_internal.h"
#include "overlay_lane.h"

namespace lt {
namespace {

// tap_in, lane_value, blend_green: overlay_lane.h (shared with k_inplace.hip)

// One thread per camera pixel; `spans` = (lo, hi) int16 per bird's-eye row of this slot.
__device__ __forceinline__ void overlay_lane_body(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out,
                                                  size_t frame_stride, const int16_t* __restrict__ oxy,
                                                  const uint16_t* __restrict__ ofrac,
                                                  const short2* __restrict__ spans, size_t span_stride, int npix,
                                                  int bh, int bw, float alpha) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= npix) return;
    const uint8_t* src = frames + (size_t)blockIdx.z * frame_stride + (size_t)o * 3;
    uint8_t* dst = out + (size_t)blockIdx.z * frame_stride + (size_t)o * 3;
    const int sx = oxy[2 * o], sy = oxy[2 * o + 1];
    const int v = lane_value(spans + (size_t)blockIdx.z * span_stride, bh, bw, sx, sy, ofrac[o]);
    const uint32_t r = src[0], g = src[1], b = src[2];
    dst[0] = (uint8_t)r;
    dst[1] = (uint8_t)(v ? blend_green(g, v, alpha) : g);
    dst[2] = (uint8_t)b;
}

__global__ __launch_bounds__(256) void k_overlay_lane(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out,
                                                     size_t frame_stride, const int16_t* __restrict__ oxy,
                                                     const uint16_t* __restrict__ ofrac,
                                                     const short2* __restrict__ spans, size_t span_stride, int npix,
                                                     int bh, int bw, float alpha) {
    overlay_lane_body(frames, out, frame_stride, oxy, ofrac, spans, span_stride, npix, bh, bw, alpha);
}
// The table-per-slot forms (_cal, here and below): frame blockIdx.z with the inverse-warp tables of its own calibration set (SlotOv).
// A pixel outside its own set's lane rows has lane value 0 -- all four taps miss the bird's-eye image -- and stays the camera pixel.
__global__ __launch_bounds__(256) void k_overlay_lane_cal(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out,
                                                         size_t frame_stride, const OvTables* __restrict__ sets, CalIds ids,
                                                         const short2* __restrict__ spans, size_t span_stride, int npix,
                                                         int bh, int bw, float alpha) {
    const OvTables& t = SlotOv{sets, &ids}.of((int)blockIdx.z);
    overlay_lane_body(frames, out, frame_stride, t.oxy, t.ofrac, spans, span_stride, npix, bh, bw, alpha);
}

// Four pixels (12 bytes = three dwords) per thread when the row length allows it.
__device__ __forceinline__ void overlay_lane4_body(const uint32_t* __restrict__ frames, uint32_t* __restrict__ out,
                                                   size_t frame_stride_dw, size_t out_stride_dw, int out_q0,
                                                   const int16_t* __restrict__ oxy,
                                                   const uint16_t* __restrict__ ofrac,
                                                   const short2* __restrict__ spans, size_t span_stride, int qa, int na,
                                                   int qb, int nb, int bh, int bw, float alpha) {
    // two runs of pixel quads per frame, [qa, qa + na) and [qb, qb + nb): the whole frame and nothing, or the text rows and
    // the rows the lane can reach (the other rows of the annotated frame are then nobody's business)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= na + nb) return;
    const int q = t < na ? qa + t : qb + (t - na);
    const uint32_t* src = frames + (size_t)blockIdx.z * frame_stride_dw + (size_t)q * 3;
    // the annotated frame at the camera frame's place (out_stride_dw = frame_stride_dw, out_q0 = 0), or -- strip mode -- only the
    // run of rows the lane can reach, packed: slot z's strip starts at z * out_stride_dw and holds the quads from out_q0 on
    uint32_t* dst = out + (size_t)blockIdx.z * out_stride_dw + (size_t)(q - out_q0) * 3;
    uint32_t d0 = src[0], d1 = src[1], d2 = src[2];
    const uint4 xy = reinterpret_cast<const uint4*>(oxy)[q];
    const uint2 fr = reinterpret_cast<const uint2*>(ofrac)[q];
    const uint32_t xyv[4] = {xy.x, xy.y, xy.z, xy.w};
    const uint32_t frv[4] = {fr.x & 0xffffu, fr.x >> 16, fr.y & 0xffffu, fr.y >> 16};
    const short2* sp = spans + (size_t)blockIdx.z * span_stride;
    int v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        v[i] = lane_value(sp, bh, bw, (int16_t)(xyv[i] & 0xffffu), (int16_t)(xyv[i] >> 16), (int)frv[i]);
    // byte layout of the three dwords: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
    if (v[0]) d0 = (d0 & 0xffff00ffu) | (blend_green((d0 >> 8) & 255u, v[0], alpha) << 8);
    if (v[1]) d1 = (d1 & 0xffffff00u) | blend_green(d1 & 255u, v[1], alpha);
    if (v[2]) d1 = (d1 & 0x00ffffffu) | (blend_green(d1 >> 24, v[2], alpha) << 24);
    if (v[3]) d2 = (d2 & 0xff00ffffu) | (blend_green((d2 >> 16) & 255u, v[3], alpha) << 16);
    dst[0] = d0;
    dst[1] = d1;
    dst[2] = d2;
}
__global__ __launch_bounds__(256) void k_overlay_lane4(const uint32_t* __restrict__ frames, uint32_t* __restrict__ out,
                                                      size_t frame_stride_dw, size_t out_stride_dw, int out_q0,
                                                      const int16_t* __restrict__ oxy,
                                                      const uint16_t* __restrict__ ofrac,
                                                      const short2* __restrict__ spans, size_t span_stride, int qa, int na,
                                                      int qb, int nb, int bh, int bw, float alpha) {
    overlay_lane4_body(frames, out, frame_stride_dw, out_stride_dw, out_q0, oxy, ofrac, spans, span_stride, qa, na, qb, nb, bh, bw, alpha);
}

__global__ __launch_bounds__(256) void k_overlay_lane4_cal(const uint32_t* __restrict__ frames, uint32_t* __restrict__ out,
                                                          size_t frame_stride_dw, const OvTables* __restrict__ sets, CalIds ids,
                                                          const short2* __restrict__ spans, size_t span_stride, int qa, int na,
                                                          int qb, int nb, int bh, int bw, float alpha) {
    const OvTables& t = SlotOv{sets, &ids}.of((int)blockIdx.z);
    overlay_lane4_body(frames, out, frame_stride_dw, frame_stride_dw, 0, t.oxy, t.ofrac, spans, span_stride, qa, na, qb, nb, bh, bw, alpha);
}

// k_overlay_lane4 for ONE frame with the row intervals as a kernel ARGUMENT (up to LT_SPAN_ARG_ROWS bird's-eye rows; should the
// runtime refuse that many argument bytes, launch_overlay_lane_one says so and the staged path takes over): process() annotates one frame per call with the host waiting for it, and intervals staged in
// page-locked memory cost a copy launch plus the events that guard the staging buffer before the overlay can start.
constexpr int SPAN_ARG_ROWS = LT_SPAN_ARG_ROWS;
struct SpanArg { short2 s[SPAN_ARG_ROWS]; };
__global__ __launch_bounds__(256) void k_overlay_lane4_arg(const uint32_t* __restrict__ frames, uint32_t* __restrict__ out,
                                                          const int16_t* __restrict__ oxy, const uint16_t* __restrict__ ofrac,
                                                          int qa, int na, int qb, int nb, int bh, int bw, float alpha,
                                                          const SpanArg spans) {
    // two runs of pixel quads: [qa, qa + na) and [qb, qb + nb) (whole rows of the frame: the text rows and the rows the lane
    // can reach, or the whole frame and nothing)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= na + nb) return;
    const int q = t < na ? qa + t : qb + (t - na);
    const uint32_t* src = frames + (size_t)q * 3;
    uint32_t* dst = out + (size_t)q * 3;
    uint32_t d0 = src[0], d1 = src[1], d2 = src[2];
    const uint4 xy = reinterpret_cast<const uint4*>(oxy)[q];
    const uint2 fr = reinterpret_cast<const uint2*>(ofrac)[q];
    const uint32_t xyv[4] = {xy.x, xy.y, xy.z, xy.w};
    const uint32_t frv[4] = {fr.x & 0xffffu, fr.x >> 16, fr.y & 0xffffu, fr.y >> 16};
    int v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        v[i] = lane_value(spans.s, bh, bw, (int16_t)(xyv[i] & 0xffffu), (int16_t)(xyv[i] >> 16), (int)frv[i]);
    if (v[0]) d0 = (d0 & 0xffff00ffu) | (blend_green((d0 >> 8) & 255u, v[0], alpha) << 8);
    if (v[1]) d1 = (d1 & 0xffffff00u) | blend_green(d1 & 255u, v[1], alpha);
    if (v[2]) d1 = (d1 & 0x00ffffffu) | (blend_green(d1 >> 24, v[2], alpha) << 24);
    if (v[3]) d2 = (d2 & 0xff00ffffu) | (blend_green((d2 >> 16) & 255u, v[3], alpha) << 16);
    dst[0] = d0;
    dst[1] = d1;
    dst[2] = d2;
}

// ---- the lane polygon of a frame from its fit, on the device (process(): the overlay enqueued right behind the search) --------
// What the host does between a frame's record and the overlay's launch -- the averaged curves (LaneTracker._averages_with), their
// plot points (lt_poly_points = get_poly_points, lane_tracker.py:511-528) and the polygon's row intervals (lane_polygon_spans =
// cv2.fillPoly's hull of the edge lines per row) -- restated for ONE workgroup that runs behind the search kernel and reads
// the fit from the slot's record: the same f64 operations in the same order (this file is built with -ffp-contract=off), the
// same integer line walk.  The overlay kernel behind it then finds the intervals in device memory, 40 us before the host could have
// launched it.  A record without a usable fit (nothing detected, a rank-deficient side: the host refits those) leaves empty
// intervals -- the frame's rows come back as they are and the host draws whatever it decides on.
struct LaneFromFit {
    double prev_sum[6];   // sum, in order, of the older fits that stay in the running average (left a, b, c; right a, b, c)
    int count;            // fits in the average, this frame's included (>= 1)
    int n_rows;           // plot rows (ploty, ploty ** 2 of get_poly_points)
    int bh, bw;           // bird's-eye size
};

__device__ __forceinline__ void dev_span_point(int* lo, int* hi, int bh, int x, int y) {
    if (y >= 0 && y < bh) {
        const int xc = min(max(x, -32768), 32767);
        atomicMin(&lo[y], xc);
        atomicMax(&hi[y], xc);
    }
}
// OpenCV's LineIterator as lt_present.cpp::span_line walks it (left end point first, error term dx - 2 dy)
__device__ void dev_span_line(int* lo, int* hi, int bh, int xa, int ya, int xb, int yb) {
    if (xb < xa) { const int tx = xa; xa = xb; xb = tx; const int ty = ya; ya = yb; yb = ty; }
    const int adx = xb - xa, ady = abs(yb - ya), ystep = yb < ya ? -1 : 1;
    const bool tall = ady > adx;
    const int len = tall ? ady : adx, across = tall ? adx : ady;
    int err = len - 2 * across;
    for (int i = 0, x = xa, y = ya; i <= len; ++i) {
        dev_span_point(lo, hi, bh, x, y);
        const bool turn = err < 0;
        err -= 2 * across;
        if (turn) err += 2 * len;
        if (tall) { y += ystep; x += turn ? 1 : 0; }
        else { x += 1; y += turn ? ystep : 0; }
    }
}

constexpr int LFF_T = 256, LFF_LONG = 64;
// One workgroup per frame.  from_region = 0 (process(): one frame): the fit comes from *rec and is averaged with p.prev_sum / p.count.
// from_region = 1 (a window's piece, lt_overlay_run_strip_coeffs): frame blockIdx.x finds its six AVERAGED coefficients and a
// "draw" byte at the start of its own interval region (the host staged them there instead of intervals) and overwrites the region.
__global__ __launch_bounds__(LFF_T) void k_lane_spans_from_fit(const lt_lane_record* __restrict__ rec, LaneFromFit p,
                                                                const double* __restrict__ ploty, const double* __restrict__ ploty2,
                                                                short2* spans_all, size_t span_stride_rows, int from_region) {
    short2* spans = spans_all + (size_t)blockIdx.x * span_stride_rows;
    extern __shared__ int s_i[];              // lo[bh], hi[bh], px[2][n_rows]
    int* lo = s_i;
    int* hi = lo + p.bh;
    int* px = hi + p.bh;
    __shared__ double s_avg[6];
    __shared__ int s_wave[LFF_T / 64], s_cnt[2], s_long[LFF_LONG], s_nlong;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool usable = from_region ? reinterpret_cast<const uint8_t*>(spans)[48] != 0 : (rec->detected != 0 && rec->fit_flags == 0);
    for (int y = tid; y < p.bh; y += LFF_T) { lo[y] = 32767; hi[y] = -32768; }
    if (tid < 6) {
        if (from_region) s_avg[tid] = reinterpret_cast<const double*>(spans)[tid];
        else {
            const double fit = tid < 3 ? rec->left_coeffs[tid] : rec->right_coeffs[tid - 3];
            const double acc = p.count > 1 ? p.prev_sum[tid] + fit : fit;  // _mean_of_rows: the sum in order, this frame's fit last,
            s_avg[tid] = acc / (double)p.count;                              // then one division by the count
        }
    }
    __syncthreads();
    if (usable) {
        const double xmax = (double)(p.bw - 1);
        for (int side = 0; side < 2; ++side) {
            const double a = s_avg[3 * side], b = s_avg[3 * side + 1], c = s_avg[3 * side + 2];
            int base = 0;                                                    // points of this side kept so far (uniform)
            for (int r0 = 0; r0 < p.n_rows; r0 += LFF_T) {
                const int r = r0 + tid;
                bool in = false;
                int xi = 0;
                if (r < p.n_rows) {
                    const double t1 = a * ploty2[r], t2 = b * ploty[r];
                    const double x = (t1 + t2) + c;
                    in = x <= xmax && x >= 0.0;
                    if (in) xi = (int)(long long)x;
                }
                const unsigned long long m = __ballot(in);
                if (lane == 0) s_wave[wv] = __popcll(m);
                __syncthreads();
                int before = 0, total = 0;
                for (int q = 0; q < LFF_T / 64; ++q) { if (q < wv) before += s_wave[q]; total += s_wave[q]; }
                if (in) px[side * p.n_rows + base + before + __popcll(m & ((1ull << lane) - 1ull))] = xi;
                base += total;
                __syncthreads();
            }
            if (tid == 0) s_cnt[side] = base;
        }
        __syncthreads();
        // the closed polygon: the left points in order, then the right points reversed; every vertex is the end point of the edge
        // before it (lane_polygon_spans)
        const int nl = s_cnt[0], nr = s_cnt[1], np = nl + nr;
        auto vertex = [&](int i, int& x, int& y) {
            if (i < nl) { x = px[i]; y = p.bh - nl + i; }
            else { const int k = nr - 1 - (i - nl); x = px[p.n_rows + k]; y = p.bh - nr + k; }
        };
        // Long edges -- the two that close the polygon run across the lane, a few hundred pixels each -- are set aside and walked by
        // the whole workgroup: pixel i of the iterator in closed form (turns before step i: T_i = max(0, ceil((2 across i - len)
        // / (2 len))), from err_i = len - 2 across (i + 1) + 2 len T_i; held against the walk for 200 000 random lines)
        if (tid == 0) s_nlong = 0;
        __syncthreads();
        for (int e = tid; e < np; e += LFF_T) {
            int x0, y0, x1, y1;
            vertex(e == 0 ? np - 1 : e - 1, x0, y0);
            vertex(e, x1, y1);
            const int adx = abs(x1 - x0), ady = abs(y1 - y0);
            if (adx <= 1 && ady <= 1) dev_span_point(lo, hi, p.bh, x1, y1);
            else if (max(adx, ady) <= 16) dev_span_line(lo, hi, p.bh, x0, y0, x1, y1);
            else {
                const int k = atomicAdd(&s_nlong, 1);
                if (k < LFF_LONG) s_long[k] = e;
                else dev_span_line(lo, hi, p.bh, x0, y0, x1, y1);
            }
        }
        __syncthreads();
        const int nlong = min(s_nlong, LFF_LONG);
        for (int k = 0; k < nlong; ++k) {
            const int e = s_long[k];
            int xa, ya, xb, yb;
            vertex(e == 0 ? np - 1 : e - 1, xa, ya);
            vertex(e, xb, yb);
            if (xb < xa) { const int tx = xa; xa = xb; xb = tx; const int ty = ya; ya = yb; yb = ty; }
            const int adx = xb - xa, ady = abs(yb - ya), ystep = yb < ya ? -1 : 1;
            const bool tall = ady > adx;
            const int len = tall ? ady : adx, across = tall ? adx : ady;
            for (int i = tid; i <= len; i += LFF_T) {
                const long long num = 2ll * across * i - len;
                const int T = num <= 0 ? 0 : (int)((num + 2ll * len - 1) / (2ll * len));
                if (tall) dev_span_point(lo, hi, p.bh, xa + T, ya + ystep * i);
                else dev_span_point(lo, hi, p.bh, xa + i, ya + ystep * T);
            }
        }
        __syncthreads();
    }
    for (int y = tid; y < p.bh; y += LFF_T) spans[y] = make_short2((short)lo[y], (short)hi[y]);
}

// Bird's-eye RGB of the undistorted rows (same taps and blend as k_warp_split, colour kept).
__global__ __launch_bounds__(256) void k_warp_rgb(const uint32_t* __restrict__ und, size_t und_px, int first_slot,
                                                 const int16_t* __restrict__ wxy, const uint16_t* __restrict__ wfrac,
                                                 FrontEndGeom g, uint8_t* __restrict__ bev, size_t bev_stride) {
    const size_t npix = (size_t)g.warp_h * g.warp_w;
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= npix) return;
    const uint32_t* src = und + und_slot_base(und_px, first_slot + (int)blockIdx.z);   // pixels of a slot are two dwords apart
    const int sx = wxy[o * 2], sy = wxy[o * 2 + 1], f = wfrac[o];
    const int fx = f & 31, fy = f >> 5, gx = 32 - fx, gy = 32 - fy;
    const int ry0 = sy - g.r0, ry1 = sy + 1 - g.r0;
    const bool y0 = sy >= 0 && sy < g.img_h && ry0 >= 0 && ry0 < g.nrows;
    const bool y1 = sy + 1 >= 0 && sy + 1 < g.img_h && ry1 >= 0 && ry1 < g.nrows;
    const bool x0 = sx >= 0 && sx < g.img_w, x1 = sx + 1 >= 0 && sx + 1 < g.img_w;
    const int cy0 = min(max(ry0, 0), g.nrows - 1), cy1 = min(max(ry1, 0), g.nrows - 1);
    const int cx0 = min(max(sx, 0), g.img_w - 1), cx1 = min(max(sx + 1, 0), g.img_w - 1);
    uint32_t t00 = src[2 * (__mul24(cy0, g.img_w) + cx0)], t01 = src[2 * (__mul24(cy0, g.img_w) + cx1)];
    uint32_t t10 = src[2 * (__mul24(cy1, g.img_w) + cx0)], t11 = src[2 * (__mul24(cy1, g.img_w) + cx1)];
    t00 = (y0 && x0) ? t00 : 0u;
    t01 = (y0 && x1) ? t01 : 0u;
    t10 = (y1 && x0) ? t10 : 0u;
    t11 = (y1 && x1) ? t11 : 0u;
    uint8_t* dst = bev + (size_t)blockIdx.z * bev_stride + o * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int h0 = __mul24((int)((t00 >> (8 * ch)) & 255u), gx) + __mul24((int)((t01 >> (8 * ch)) & 255u), fx);
        const int h1 = __mul24((int)((t10 >> (8 * ch)) & 255u), gx) + __mul24((int)((t11 >> (8 * ch)) & 255u), fx);
        dst[ch] = (uint8_t)((__mul24(h0, gy) + __mul24(h1, fy) + 512) >> 10);
    }
}

// Text lines blended in white onto the annotated frames from a glyph atlas (one alpha cell of gw x gh bytes
// per character; the cell of character ch is used up to its advance width).  One thread per cell pixel of
// every character of every line: lines[(slot * nl + line) * len + k] is the character, xpos[...] its left edge.
__global__ __launch_bounds__(256) void k_overlay_text(uint8_t* __restrict__ out, size_t frame_stride, int img_h, int img_w,
                                                     const uint8_t* __restrict__ atlas, const uint8_t* __restrict__ advance,
                                                     int first_char, int n_glyphs, int gw, int gh,
                                                     const uint8_t* __restrict__ lines, const int16_t* __restrict__ xpos,
                                                     int nl, int len, int slot_chars, int y0, int step) {
    const int cell = gw * gh, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= len * cell) return;
    const int k = t / cell, rem = t - k * cell, gy = rem / gw, gx = rem - gy * gw;
    const int line = blockIdx.y, slot = blockIdx.z;
    const size_t li = (size_t)slot * slot_chars + (size_t)line * len + k;     // a slot's lines sit at the buffers' fixed stride
    const int ch = (int)lines[li] - first_char;
    if (ch < 0 || ch >= n_glyphs || gx >= advance[ch]) return;
    const int alpha = atlas[((size_t)ch * gh + gy) * gw + gx];
    if (alpha == 0) return;
    const int x = xpos[li] + gx, y = y0 + line * step + gy;
    if (x < 0 || x >= img_w || y < 0 || y >= img_h) return;
    uint8_t* px = out + (size_t)slot * frame_stride + ((size_t)y * img_w + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = px[c];
        px[c] = (uint8_t)(v + ((255 - v) * alpha + 127) / 255);      // white over the frame
    }
}

}  // namespace

// Small host -> device copies of the overlay stage as a KERNEL reading page-locked (device-visible) host memory: a
// hipMemcpyAsync of a few hundred KB was seen to block its caller for as long as a large upload on another stream was in
// progress (8 ms per window); a launch never waits.
namespace {
__global__ __launch_bounds__(256) void k_copy_words(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
}  // namespace

void launch_copy_from_pinned(hipStream_t s, void* dst, const void* src_pinned, size_t bytes) {
    if (!bytes) return;
    void* src_dev = nullptr;
    if (((bytes | (size_t)(uintptr_t)dst | (size_t)(uintptr_t)src_pinned) & 3) ||
        hipHostGetDevicePointer(&src_dev, const_cast<void*>(src_pinned), 0) != hipSuccess || !src_dev) {
        (void)hipMemcpyAsync(dst, src_pinned, bytes, hipMemcpyHostToDevice, s);
        return;
    }
    const size_t n = bytes >> 2;
    hipLaunchKernelGGL(k_copy_words, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, static_cast<uint32_t*>(dst),
                       static_cast<const uint32_t*>(src_dev), n);
}

// A few words or kilobytes device -> page-locked host memory as a kernel launch (records, lane-pixel blocks): a hipMemcpyAsync
// of 64 bytes takes 23 us by itself and, beside a stream of annotated frames, queues behind them on the copy engine (4 ms per
// lt_download_pixels in an annotated 1920x1080 stream); a launch does neither.  false: not word-aligned / not page-locked.
bool launch_copy_words_to_pinned(hipStream_t s, void* dst_pinned, const void* src, size_t bytes) {
    if (!bytes) return true;
    void* dst_dev = nullptr;
    if (((bytes | (size_t)(uintptr_t)dst_pinned | (size_t)(uintptr_t)src) & 3) ||
        hipHostGetDevicePointer(&dst_dev, dst_pinned, 0) != hipSuccess || !dst_dev) {
        (void)hipGetLastError();
        return false;
    }
    const size_t n = bytes >> 2;
    hipLaunchKernelGGL(k_copy_words, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, static_cast<uint32_t*>(dst_dev),
                       static_cast<const uint32_t*>(src), n);
    return true;
}

// One lane record (64 bytes = 16 words) into its page-locked mirror, and behind it the ticket the host polls (the word after the
// record): what k_band_chain3 does for a one-frame band search by itself, for the one-frame SLIDING-WINDOW search (the first frame of
// a video, every frame while the detector is lost: lane_tracker.py:851) -- lt_download_records then polls instead of waiting for
// the stream, which returns 15-20 us after the data is there.  One wave: the fence in front of the ticket is one wave's.
namespace {
__global__ __launch_bounds__(64) void k_mirror_record(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, unsigned ticket) {
    if (threadIdx.x < 16) dst[threadIdx.x] = src[threadIdx.x];
    __threadfence_system();
    if (threadIdx.x == 0) *reinterpret_cast<volatile unsigned*>(dst + 16) = ticket;
}
}  // namespace
bool launch_mirror_record(hipStream_t s, void* dst_pinned, const void* src_record, unsigned ticket) {
    void* dst_dev = nullptr;
    if (hipHostGetDevicePointer(&dst_dev, dst_pinned, 0) != hipSuccess || !dst_dev) {
        (void)hipGetLastError();
        return false;
    }
    hipLaunchKernelGGL(k_mirror_record, dim3(1), dim3(64), 0, s, static_cast<uint32_t*>(dst_dev), static_cast<const uint32_t*>(src_record), ticket);
    return true;
}

// Device -> page-locked host memory by a kernel (16 bytes per lane, grid-stride over a grid that a few CUs hold), the
// alternative to the copy engine for lt_download_overlay_async (LT_DL_KERNEL=1; trade-off and numbers there and in
// tools/microbench/d2h_kernel.hip): stores from a kernel cross the bus beside the engine's uploads whatever engine the runtime
// gave the download stream.
namespace {
typedef unsigned int vec4u __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_copy_vec16(vec4u* __restrict__ dst, const vec4u* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}
}  // namespace

// The same for one run of rows of n frames: bytes [off, off + bytes) of every frame, the frames `pitch` bytes apart in both
// buffers (lt_download_overlay_rows_async).
namespace {
__global__ __launch_bounds__(256) void k_copy_rows16(vec4u* __restrict__ dst, const vec4u* __restrict__ src, unsigned pitch16,
                                                    unsigned off16, unsigned w16, unsigned total) {
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const unsigned f = i / w16, u = i - f * w16;
        const size_t a = (size_t)f * pitch16 + off16 + u;
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + a), dst + a);
    }
}
}  // namespace

bool launch_copy_rows_to_pinned(hipStream_t s, void* dst_pinned, const void* src, size_t pitch, size_t off, size_t bytes, int n) {
    if (!bytes || n <= 0) return true;
    void* dst_dev = nullptr;
    const size_t total = (size_t)n * (bytes >> 4);
    if (((bytes | pitch | off | (size_t)(uintptr_t)dst_pinned | (size_t)(uintptr_t)src) & 15) || total >= 0xffffffffull ||
        (pitch >> 4) >= 0xffffffffull || hipHostGetDevicePointer(&dst_dev, dst_pinned, 0) != hipSuccess || !dst_dev) {
        (void)hipGetLastError();
        return false;
    }
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 64);
    hipLaunchKernelGGL(k_copy_rows16, dim3(blocks), dim3(256), 0, s, static_cast<vec4u*>(dst_dev), static_cast<const vec4u*>(src),
                       (unsigned)(pitch >> 4), (unsigned)(off >> 4), (unsigned)(bytes >> 4), (unsigned)total);
    return true;
}

bool launch_copy_to_pinned(hipStream_t s, void* dst_pinned, const void* src, size_t bytes) {
    if (!bytes) return true;
    void* dst_dev = nullptr;
    if (((bytes | (size_t)(uintptr_t)dst_pinned | (size_t)(uintptr_t)src) & 15) ||
        hipHostGetDevicePointer(&dst_dev, dst_pinned, 0) != hipSuccess || !dst_dev) {
        (void)hipGetLastError();
        return false;                    // not page-locked (or not aligned): the caller copies with hipMemcpyAsync
    }
    const size_t n = bytes >> 4;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 64);   // 64 blocks already saturate the bus (tools/microbench/d2h_kernel.hip)
    hipLaunchKernelGGL(k_copy_vec16, dim3(blocks), dim3(256), 0, s, static_cast<vec4u*>(dst_dev), static_cast<const vec4u*>(src), n);
    return true;
}

void launch_overlay_text(hipStream_t s, uint8_t* out, size_t frame_stride, int img_h, int img_w, const uint8_t* atlas,
                         const uint8_t* advance, int first_char, int n_glyphs, int gw, int gh, const uint8_t* lines,
                         const int16_t* xpos, int nl, int len, int slot_chars, int y0, int step, int n) {
    if (n <= 0 || nl <= 0 || len <= 0) return;
    dim3 grid((unsigned)((len * gw * gh + 255) / 256), (unsigned)nl, (unsigned)n);
    hipLaunchKernelGGL(k_overlay_text, grid, dim3(256), 0, s, out, frame_stride, img_h, img_w, atlas, advance, first_char,
                       n_glyphs, gw, gh, lines, xpos, nl, len, slot_chars, y0, step);
}

bool launch_overlay_lane_strip(hipStream_t s, const uint8_t* frames, size_t frame_stride, uint8_t* strips, size_t strip_stride,
                               const int16_t* oxy, const uint16_t* ofrac, const int16_t* spans, size_t span_stride_rows, int img_w,
                               int row0, int row1, int bh, int bw, float alpha, int n) {
    if (n <= 0 || row1 <= row0) return true;
    if ((img_w & 3) || (frame_stride & 3) || (strip_stride & 3) || (((size_t)(uintptr_t)frames | (size_t)(uintptr_t)strips) & 3)) return false;
    const int qrow = img_w >> 2, qb = row0 * qrow, nb = (row1 - row0) * qrow;
    hipLaunchKernelGGL(k_overlay_lane4, dim3((nb + 255) / 256, 1, n), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(frames),
                       reinterpret_cast<uint32_t*>(strips), frame_stride >> 2, strip_stride >> 2, qb, oxy, ofrac,
                       reinterpret_cast<const short2*>(spans), span_stride_rows, 0, 0, qb, nb, bh, bw, alpha);
    return true;
}

// two runs of camera rows r = {a0, a1, b0, b1} (nullptr: the whole frame) as runs of pixel quads [qa, qa + na), [qb, qb + nb)
struct QuadRuns { int qa, na, qb, nb; };
static QuadRuns quad_runs(const int* r, int img_h, int img_w) {
    const int q = img_w >> 2;
    return r ? QuadRuns{r[0] * q, (r[1] - r[0]) * q, r[2] * q, (r[3] - r[2]) * q} : QuadRuns{0, img_h * q, 0, 0};
}

int launch_overlay_lane(hipStream_t s, const uint8_t* frames, uint8_t* out, size_t frame_stride, const int16_t* oxy,
                        const uint16_t* ofrac, const int16_t* spans, size_t span_stride_rows, int img_h, int img_w,
                        int bh, int bw, float alpha, int n, const int* rows4, OvSets per_slot) {
    if (n <= 0) return 0;
    const int npix = img_h * img_w;
    const short2* sp = reinterpret_cast<const short2*>(spans);
    const bool four = (img_w & 3) == 0 && (frame_stride & 3) == 0;
    const auto [qa, na, qb, nb] = quad_runs(rows4, img_h, img_w);
    if (four && na + nb <= 0) return 0;
    if (per_slot.sets) {         // every slot with the tables of its own set: CalIds::N slots per launch
        int launches = 0;
        for (int at = 0; at < n; at += CalIds::N, ++launches) {
            const int m = std::min(n - at, (int)CalIds::N);
            const CalIds ids = pack_cal_ids(per_slot.ids + at, m);
            const uint8_t* f = frames + (size_t)at * frame_stride;
            uint8_t* o = out + (size_t)at * frame_stride;
            const short2* spz = sp + (size_t)at * span_stride_rows;
            if (four)
                hipLaunchKernelGGL(k_overlay_lane4_cal, dim3((na + nb + 255) / 256, 1, m), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(f),
                                   reinterpret_cast<uint32_t*>(o), frame_stride >> 2, per_slot.sets, ids, spz, span_stride_rows, qa, na, qb, nb, bh, bw, alpha);
            else
                hipLaunchKernelGGL(k_overlay_lane_cal, dim3((npix + 255) / 256, 1, m), dim3(256), 0, s, f, o, frame_stride, per_slot.sets, ids, spz,
                                   span_stride_rows, npix, bh, bw, alpha);
        }
        return launches;
    }
    if (four) {
        hipLaunchKernelGGL(k_overlay_lane4, dim3((na + nb + 255) / 256, 1, n), dim3(256), 0, s,
                           reinterpret_cast<const uint32_t*>(frames), reinterpret_cast<uint32_t*>(out), frame_stride >> 2, frame_stride >> 2, 0,
                           oxy, ofrac, sp, span_stride_rows, qa, na, qb, nb, bh, bw, alpha);
    } else {      // (a row length that is no multiple of 4: the whole frame whatever the runs -- a superset)
        hipLaunchKernelGGL(k_overlay_lane, dim3((npix + 255) / 256, 1, n), dim3(256), 0, s, frames, out, frame_stride, oxy,
                           ofrac, sp, span_stride_rows, npix, bh, bw, alpha);
    }
    return 1;
}

bool launch_overlay_lane_one(hipStream_t s, const uint8_t* frame, uint8_t* out, const int16_t* oxy, const uint16_t* ofrac,
                             const int16_t* spans_host, int img_h, int img_w, int bh, int bw, float alpha, const int* rows4) {
    static bool refused = false;         // the runtime did not take a launch with this many argument bytes: never again
    if (refused || bh > SPAN_ARG_ROWS || (img_w & 3) || (((size_t)(uintptr_t)frame | (size_t)(uintptr_t)out) & 3)) return false;
    SpanArg arg;
    std::memcpy(arg.s, spans_host, (size_t)bh * sizeof(short2));
    const auto [qa, na, qb, nb] = quad_runs(rows4, img_h, img_w);
    if (na + nb <= 0) return true;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_overlay_lane4_arg, dim3((na + nb + 255) / 256), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(frame),
                       reinterpret_cast<uint32_t*>(out), oxy, ofrac, qa, na, qb, nb, bh, bw, alpha, arg);
    if (hipGetLastError() != hipSuccess) { refused = true; return false; }
    return true;
}

// one word into (page-locked, device-visible) memory behind everything enqueued on `s` so far: a ticket the host polls instead of
// waiting for the stream (hipStreamSynchronize on a stream with a dozen finished launches costs 15-20 us of bookkeeping)
namespace { __global__ void k_store_word(volatile unsigned* p, unsigned v) { __threadfence_system(); *p = v; } }
void launch_store_word(hipStream_t s, unsigned* dev_word, unsigned value) {
    hipLaunchKernelGGL(k_store_word, dim3(1), dim3(1), 0, s, dev_word, value);
}

// row intervals of the averaged lane of the frame whose record is *rec (k_lane_spans_from_fit); false: too many rows for the LDS
// the same for n frames whose averaged coefficients (6 doubles) and draw byte (offset 48) stand at the start of their interval regions
static size_t lane_spans_lds(int bh, int n_rows) { return ((size_t)2 * bh + (size_t)2 * std::max(n_rows, 1)) * sizeof(int); }
bool lane_spans_from_regions_available(int bh, int n_rows) {
    return n_rows >= 0 && (bh & 1) == 0 && bh * 4 >= 56 && lane_spans_lds(bh, n_rows) <= 60 * 1024;   // (regions of 4 bh bytes: 8-byte aligned, >= 56 bytes)
}
bool launch_lane_spans_from_regions(hipStream_t s, const double* ploty, const double* ploty2, int n_rows, int bh, int bw, int16_t* spans,
                                    int n) {
    if (n < 1 || !lane_spans_from_regions_available(bh, n_rows)) return false;
    const size_t lds = lane_spans_lds(bh, n_rows);
    LaneFromFit p;
    for (int k = 0; k < 6; ++k) p.prev_sum[k] = 0.0;
    p.count = 1;
    p.n_rows = n_rows;
    p.bh = bh;
    p.bw = bw;
    hipLaunchKernelGGL(k_lane_spans_from_fit, dim3(n), dim3(LFF_T), lds, s, (const lt_lane_record*)nullptr, p, ploty, ploty2,
                       reinterpret_cast<short2*>(spans), (size_t)bh, 1);
    return true;
}

bool launch_lane_spans_from_fit(hipStream_t s, const lt_lane_record* rec, const double* prev_sum, int count, const double* ploty,
                                const double* ploty2, int n_rows, int bh, int bw, int16_t* spans) {
    const size_t lds = lane_spans_lds(bh, n_rows);
    if (lds > 60 * 1024 || count < 1 || n_rows < 0) return false;
    LaneFromFit p;
    for (int k = 0; k < 6; ++k) p.prev_sum[k] = prev_sum ? prev_sum[k] : 0.0;
    p.count = count;
    p.n_rows = n_rows;
    p.bh = bh;
    p.bw = bw;
    hipLaunchKernelGGL(k_lane_spans_from_fit, dim3(1), dim3(LFF_T), lds, s, rec, p, ploty, ploty2, reinterpret_cast<short2*>(spans), (size_t)bh, 0);
    return true;
}

void launch_warp_rgb(hipStream_t s, const uint32_t* und, size_t und_px, int first_slot, const int16_t* wxy, const uint16_t* wfrac,
                     FrontEndGeom g, uint8_t* bev, size_t bev_stride, int n) {
    if (n <= 0) return;
    const size_t npix = (size_t)g.warp_h * g.warp_w;
    hipLaunchKernelGGL(k_warp_rgb, dim3((unsigned)((npix + 255) / 256), 1, n), dim3(256), 0, s, und, und_px, first_slot, wxy,
                       wfrac, g, bev, bev_stride);
}

// Code objects load on the first launch of one of their kernels (a few ms each, once per process and device): lt_create launches
// this no-op so that no stream's first window pays for it (lt_api.cpp: preload_kernels).
namespace { __global__ void k_preload_k_overlay() {} }
void preload_k_overlay(hipStream_t s) { hipLaunchKernelGGL(k_preload_k_overlay, dim3(1), dim3(1), 0, s); }

}  // namespace lt

