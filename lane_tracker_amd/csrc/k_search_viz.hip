// The search visualisations (lane_tracker.py:687-771) and cv2.resize(INTER_LINEAR) on u8 images, on the device:
//   k_search_viz         one pass over the picture, every pixel decides its own colour: the mask, the search windows or bands in
//                        transparent green, the lane pixels where the slot's list region holds them as column masks (forms 1, 2)
//   k_search_viz_points  what comes as lists: the lane pixels of the packed form (0), left before right, then the fitted curves
//   k_resize_linear_u8   half-pixel centres, 11-bit coefficients, OpenCV's two-stage rounding (utils.resize_linear), tables from the host
// Pictures equal overlay.visualize_sliding_window_search / visualize_band_search bit for bit (tests/test_gpu_search_viz.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "lt_internal.h"

namespace lt {
namespace {

// cv2.addWeighted(a, 1, b, beta, 0) on u8: f32 products and sums, round-half-even, saturate (overlay.add_weighted)
__device__ inline unsigned blend_u8(unsigned a, unsigned b, float beta) {
    float t = __fadd_rn(__fmul_rn((float)a, 1.0f), __fmul_rn((float)b, beta));
    t = __fadd_rn(t, 0.0f);
    t = rintf(t);
    return (unsigned)fminf(fmaxf(t, 0.0f), 255.0f);
}

__device__ inline bool in_span(const int16_t* band, int h, int y, int x) {      // either side's clipped interval of row y
    const int l0 = band[2 * y], l1 = band[2 * y + 1], r0 = band[2 * (h + y)], r1 = band[2 * (h + y) + 1];
    return (x >= l0 && x <= l1) || (x >= r0 && x <= r1);
}

// The lane pixels of row y as one 64-bit column mask and a first column per side, from the slot's list region in the form the
// record's reserved byte names (lt_internal.h: sws2_* / band2_*); a region whose header does not fit the buffer gives none.
__device__ inline void row_members(const uint32_t* pix, unsigned form, int maxpix, int y, int a[2], unsigned long long m[2]) {
    a[0] = a[1] = 0;
    m[0] = m[1] = 0ull;
    if (form == 1) {
        const int nlev = (int)pix[0], wh = (int)pix[1], H1 = (int)pix[2];
        if (nlev < 1 || wh < 1 || sws2_block_words(nlev, wh) > 2LL * maxpix || y >= H1) return;
        const int level = (H1 - 1 - y) / wh;
        if (level >= nlev) return;
        const int ry = y - (H1 - (1 + level) * wh);
        const int32_t* roi = reinterpret_cast<const int32_t*>(pix + 4);
        const uint32_t* masks = pix + sws2_mask_offset(nlev);
        for (int side = 0; side < 2; ++side) {
            const int sl = side * nlev + level;
            if (roi[2 * sl + 1] <= roi[2 * sl]) continue;
            const size_t mi = ((size_t)sl * wh + ry) * 2;
            a[side] = roi[2 * sl];
            m[side] = (unsigned long long)masks[mi] | ((unsigned long long)masks[mi + 1] << 32);
        }
    } else if (form == 2) {
        const int nrows = (int)pix[0], top = (int)pix[1];
        if (nrows < 1 || band2_block_words(nrows) > 2LL * maxpix || y < top || y - top >= nrows) return;
        const int ry = y - top;
        const int32_t* row_a = reinterpret_cast<const int32_t*>(pix + 4);
        const uint32_t* masks = pix + band2_mask_offset(nrows);
        for (int side = 0; side < 2; ++side) {
            const size_t mi = ((size_t)side * nrows + ry) * 2;
            a[side] = row_a[(size_t)side * nrows + ry];
            m[side] = (unsigned long long)masks[mi] | ((unsigned long long)masks[mi + 1] << 32);
        }
    }
}

// grid (h, frames): a workgroup paints one row, a lane four pixels at a time = three dwords
__global__ void k_search_viz(VizBatch b, int h, int w, int wpr, int maxpix, int maxlev) {
    const VizFrame& f = b.f[blockIdx.y];
    const int y = (int)blockIdx.x;
    const int kind = f.kind;
    // what the row is made of: the same for every lane
    int win[2][2] = {{0, 0}, {0, 0}};          // kind 1: columns [lo, hi) of the left / right window over this row
    if (kind == 1 && y < f.H1) {
        const int level = (f.H1 - 1 - y) / f.wh;
        if (f.H1 - (level + 1) * f.wh >= 0) {       // (a window that sticks out above the image is an empty slice upstream)
            for (int side = 0; side < 2; ++side) {
                const int32_t* t = f.cent + (size_t)side * (maxlev + 2);
                const int n = min(max(t[0], 0), maxlev + 1);
                if (level >= n) continue;
                const double center = (double)t[1 + level], half = (double)f.ww / 2.0;
                int hi = min((int)(center + half), w);
                if (hi < 0) hi = max(hi + w, 0);    // (a negative slice end counts from the right)
                win[side][0] = max((int)(center - half), 0);
                win[side][1] = hi;
            }
        }
    }
    int ma[2] = {0, 0};
    unsigned long long mm[2] = {0ull, 0ull};
    if (kind != 0) row_members(f.pix, f.rec->_pad, maxpix, y, ma, mm);
    const bool wide = (w & 3) == 0;
    uint8_t* orow = f.out + (size_t)y * w * 3;
    for (int x0 = 4 * (int)threadIdx.x; x0 < w; x0 += 4 * (int)blockDim.x) {
        const int npx = min(4, w - x0);
        unsigned mv[4] = {0, 0, 0, 0};
        if (f.bits) {
            const unsigned long long word = f.bits[(size_t)y * wpr + (x0 >> 6)];     // x0 is a multiple of 4: one word holds the four
            const unsigned nib = (unsigned)(word >> (x0 & 63)) & 15u;
            for (int j = 0; j < 4; ++j) mv[j] = (nib >> j) & 1u ? 255u : 0u;
        } else {
            for (int j = 0; j < npx; ++j) mv[j] = f.mask[(size_t)y * w + x0 + j];
        }
        unsigned px[12];
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            unsigned r = mv[j], g = mv[j], bl = mv[j];
            const bool left = (unsigned)(x - ma[0]) < 64u && ((mm[0] >> (unsigned)(x - ma[0])) & 1ull);
            const bool right = (unsigned)(x - ma[1]) < 64u && ((mm[1] >> (unsigned)(x - ma[1])) & 1ull);
            if (kind == 1) {
                const unsigned gw = ((x >= win[0][0] && x < win[0][1] ? 255u : 0u) + (x >= win[1][0] && x < win[1][1] ? 255u : 0u)) & 255u;
                if (gw) g = blend_u8(g, gw, 0.5f);
            }
            if (left) { r = 255u; g = 0u; bl = 0u; }
            if (right) { r = 0u; g = 0u; bl = 255u; }
            if (kind == 2 && in_span(f.band, h, y, x)) g = blend_u8(g, 255u, 0.3f);      // after the lane pixels: upstream's order
            px[3 * j] = r;
            px[3 * j + 1] = g;
            px[3 * j + 2] = bl;
        }
        if (wide) {
            uint32_t* o = reinterpret_cast<uint32_t*>(orow + (size_t)x0 * 3);
            o[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
            o[1] = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
            o[2] = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
        } else {
            for (int k = 0; k < 3 * npx; ++k) orow[(size_t)x0 * 3 + k] = (uint8_t)px[k];
        }
    }
}

// grid (frames): the lists, in upstream's order of assignment -- left lane pixels, right lane pixels (form 0 only), the curves
__global__ void k_search_viz_points(VizBatch b, int h, int w, int maxpix) {
    const VizFrame& f = b.f[blockIdx.x];
    if (f.kind == 0) return;
    if (f.rec->_pad != 1 && f.rec->_pad != 2) {
        for (int side = 0; side < 2; ++side) {
            const int n = min(max(side == 0 ? f.rec->n_left : f.rec->n_right, 0), maxpix);
            const uint32_t* list = f.pix + (size_t)side * maxpix;
            for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) {
                const int y = (int)(list[i] >> 16), x = (int)(list[i] & 0xffffu);
                if (y >= h || x >= w) continue;
                uint8_t* o = f.out + ((size_t)y * w + x) * 3;
                o[0] = side == 0 ? 255 : 0;
                o[1] = (uint8_t)(f.kind == 2 && in_span(f.band, h, y, x) ? blend_u8(0u, 255u, 0.3f) : 0u);
                o[2] = side == 0 ? 0 : 255;
            }
            __syncthreads();             // the right list is painted over the left one, the curves over both
        }
    }
    const int n = f.n_fit_left + f.n_fit_right;
    for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) {
        const int y = f.pts[2 * i], x = f.pts[2 * i + 1];
        if (y < 0 || y >= h || x < 0 || x >= w) continue;
        uint8_t* o = f.out + ((size_t)y * w + x) * 3;
        o[0] = 255;
        o[1] = 235;
        o[2] = 0;
    }
}

// grid (groups of four destination columns, destination rows, images); xt / yt: per destination column / row (tap 0, tap 1, coefficient
// 0, coefficient 1).  Columns [0, dcols) of the scaled image go to columns dcol0 .. of the destination rows (dpitch bytes each).
__global__ void k_resize_linear_u8(const uint8_t* src, size_t src_stride, int sw, int ch, uint8_t* dst, size_t dst_stride, int dpitch,
                                   int dcol0, int dcols, const int4* xt, const int4* yt) {
    const int x0 = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (x0 >= dcols) return;
    const int y = (int)blockIdx.y, npx = min(4, dcols - x0);
    const int4 ty = yt[y];
    const uint8_t* s0 = src + (size_t)blockIdx.z * src_stride + (size_t)ty.x * sw * ch;
    const uint8_t* s1 = src + (size_t)blockIdx.z * src_stride + (size_t)ty.y * sw * ch;
    unsigned v[12];
    for (int j = 0; j < npx; ++j) {
        const int4 tx = xt[x0 + j];
        for (int k = 0; k < ch; ++k) {
            const int r0 = (int)s0[tx.x * ch + k] * tx.z + (int)s0[tx.y * ch + k] * tx.w;
            const int r1 = (int)s1[tx.x * ch + k] * tx.z + (int)s1[tx.y * ch + k] * tx.w;
            const int o = (((ty.z * (r0 >> 4)) >> 16) + ((ty.w * (r1 >> 4)) >> 16) + 2) >> 2;
            v[j * ch + k] = (unsigned)min(max(o, 0), 255);
        }
    }
    uint8_t* o = dst + (size_t)blockIdx.z * dst_stride + (size_t)y * dpitch + (size_t)(dcol0 + x0) * ch;
    const int nb = npx * ch;
    if (npx == 4 && ((uintptr_t)o & 3) == 0) {
        uint32_t* q = reinterpret_cast<uint32_t*>(o);
        for (int k = 0; k < ch; ++k) q[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < nb; ++k) o[k] = (uint8_t)v[k];
    }
}

__global__ void k_preload_k_search_viz() {}

}  // namespace

void launch_search_viz(hipStream_t s, const VizBatch& b, int n, int h, int w, int wpr, int maxpix, int maxlev) {
    if (n <= 0 || h <= 0 || w <= 0) return;
    const int lanes = (w + 3) / 4, block = std::min(1024, (lanes + 63) & ~63);
    hipLaunchKernelGGL(k_search_viz, dim3((unsigned)h, (unsigned)n), dim3((unsigned)block), 0, s, b, h, w, wpr, maxpix, maxlev);
    hipLaunchKernelGGL(k_search_viz_points, dim3((unsigned)n), dim3(256), 0, s, b, h, w, maxpix);
}

void launch_resize_linear_u8(hipStream_t s, const uint8_t* src, size_t src_stride, int sw, int ch, uint8_t* dst, size_t dst_stride,
                             int dpitch, int dcol0, int dcols, int dh, const int32_t* xt, const int32_t* yt, int n) {
    if (n <= 0 || dcols <= 0 || dh <= 0) return;
    const int lanes = (dcols + 3) / 4;
    hipLaunchKernelGGL(k_resize_linear_u8, dim3((unsigned)((lanes + 63) / 64), (unsigned)dh, (unsigned)n), dim3(64), 0, s, src, src_stride,
                       sw, ch, dst, dst_stride, dpitch, dcol0, dcols, reinterpret_cast<const int4*>(xt), reinterpret_cast<const int4*>(yt));
}

void preload_k_search_viz(hipStream_t s) { hipLaunchKernelGGL(k_preload_k_search_viz, dim3(1), dim3(1), 0, s); }

}  // namespace lt
