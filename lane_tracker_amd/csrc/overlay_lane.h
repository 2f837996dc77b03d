// The lane polygon as a camera pixel sees it (device code shared by k_overlay.hip and k_inplace.hip).
//
// The filled polygon is never rasterised: it is y-monotone (both lane curves are functions of y), so it is described by one
// column interval [lo, hi] per bird's-eye row (`spans`).  The inverse warp is OpenCV's fixed-point bilinear remap of that 0/255
// image: each camera pixel tests its four taps -- (sx, sy) .. (sx + 1, sy + 1) of the `oxy` table, 5-bit fractions `f` of the
// `ofrac` table -- against the row intervals.  What the value does to the pixel: inplace_arith.h (blend_green).
#pragma once
#include <hip/hip_runtime.h>

#include "inplace_arith.h"

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

}  // namespace lt
