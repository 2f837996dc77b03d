// The lane polygon and the text as a camera pixel sees them (device code shared by k_overlay.hip, k_inplace.hip and k_draw_sink.hip).
//
// The filled polygon is never rasterised: it is y-monotone (both lane curves are functions of y), so it is described by one
// column interval [lo, hi] per bird's-eye row (`spans`).  The inverse warp is OpenCV's fixed-point bilinear remap of that 0/255
// image: each camera pixel tests its four taps -- (sx, sy) .. (sx + 1, sy + 1) of the `oxy` table, 5-bit fractions `f` of the
// `ofrac` table -- against the row intervals.  What the value does to the pixel: inplace_arith.h (blend_green).
#pragma once
#include <hip/hip_runtime.h>

#include "inplace_arith.h"
#include "lt_internal.h"

namespace lt {

__device__ __forceinline__ int tap_in(const short2* __restrict__ spans, int bh, int bw, int x, int y) {
    const short2 s = spans[min(max(y, 0), bh - 1)];
    return (y >= 0 && y < bh && x >= 0 && x < bw && x >= s.x && x <= s.y) ? 255 : 0;
}

__device__ __forceinline__ int lane_value(const short2* __restrict__ spans, int bh, int bw, int sx, int sy, int f) {
    const int fx = f & 31, fy = f >> 5, gx = 32 - fx, gy = 32 - fy;
    const int v00 = tap_in(spans, bh, bw, sx, sy), v01 = tap_in(spans, bh, bw, sx + 1, sy);
    const int v10 = tap_in(spans, bh, bw, sx, sy + 1), v11 = tap_in(spans, bh, bw, sx + 1, sy + 1);
    const int h0 = __mul24(v00, gx) + __mul24(v01, fx), h1 = __mul24(v10, gx) + __mul24(v11, fx);
    return (__mul24(h0, gy) + __mul24(h1, fy) + 512) >> 10;      // == (sum w_i v_i + 2^14) >> 15
}

using ia::blend_green;

// The alpha of the glyph over pixel (x, y) of frame z, 0 where there is none.  The line comes from y0 / step / gh (lines do not
// overlap: step >= gh, checked on the host), the character from the slot's positions: xpos[] never decreases along a line (a
// running sum of advances), cells are disjoint, so the last character that starts at or before x is the only candidate.
__device__ __forceinline__ int text_alpha(const InplaceText& t, int z, int x, int y) {
    const int dy = y - t.y0;
    if (t.nl <= 0 || dy < 0) return 0;
    const int line = dy / t.step, gy = dy - line * t.step;
    if (line >= t.nl || gy >= t.gh) return 0;
    const size_t base = (size_t)z * t.slot_chars + (size_t)line * t.len;
    const int16_t* __restrict__ xp = t.xpos + base;
    int lo = 0, hi = t.len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xp[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return 0;
    const int k = lo - 1;
    const int ch = (int)t.lines[base + k] - t.first_char;
    if (ch < 0 || ch >= t.n_glyphs) return 0;
    const int gx = x - xp[k];
    if (gx >= t.advance[ch] || gx >= t.gw) return 0;
    return t.atlas[((size_t)ch * t.gh + gy) * t.gw + gx];
}

// The tables policy of the table-per-slot presentation kernels, as the front end's SlotTables: frame z of a launch takes the
// inverse-warp tables of its own calibration set -- uniform per workgroup (z is blockIdx.z), so the pair arrives by scalar loads.
struct SlotOv {
    const OvTables* sets;
    const CalIds* ids;
    __device__ __forceinline__ const OvTables& of(int z) const { return sets[(ids->w[z >> 2] >> (8 * (z & 3))) & 255u]; }
};
inline CalIds pack_cal_ids(const uint8_t* ids, int m) {
    CalIds c{};
    for (int i = 0; i < m; ++i) c.w[i >> 2] |= (uint32_t)ids[i] << (8 * (i & 3));
    return c;
}

}  // namespace lt
