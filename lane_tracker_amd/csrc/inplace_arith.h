// The presentation stage's per-pixel arithmetic -- the lane's green blend, the text's white blend, and both over a 2 x 2 block of a
// YUV 4:2:0 surface -- as plain inline functions without HIP types: k_overlay.hip and k_inplace.hip run exactly these expressions
// on the device, and a host translation unit (tests/inplace_arith_host.cpp) compiles the same header with the system compiler
// (-ffp-contract=off, as the library), so the CPU tests check what the GPU runs.
//
// A block of a 4:2:0 surface a lane or a text line lands on is converted ONCE to RGB (yuv_arith.h: the front end's conversion, what
// the camera frame is to every other route), drawn on -- lane, then text, as lt_overlay_run and lt_overlay_text follow each other --
// and converted back ONCE (sink_arith.h: what lt_overlay_store_device would write).  YUV -> RGB -> YUV is not the identity, so
// only what changed as RGB goes back: Y of a pixel whose RGB changed, (U, V) of a block whose top-left pixel's RGB changed (the
// pixel OpenCV's RGB2YUV_I420 takes chroma from).  Everything else keeps the bytes the decoder wrote.
#pragma once
#include <cmath>
#include <cstdint>

#include "sink_arith.h"
#include "yuv_arith.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define IA_HD inline
#endif

namespace lt {
namespace ia {

// cv::addWeighted(img, 1, lane, alpha, 0) of the green byte: the product rounded, then the sum (no fma), then rounded half to even
// and saturated
IA_HD uint32_t blend_green(uint32_t g, int lane, float alpha) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float t = __fadd_rn((float)g, __fmul_rn((float)lane, alpha));   // no fma: cv::addWeighted rounds the product
    const int r = (int)rintf(t);
    return (uint32_t)min(max(r, 0), 255);
#else
    volatile float p = (float)lane * alpha;                                // (volatile: the product is rounded whatever the flags)
    const float t = (float)g + p;
    const int r = (int)std::rint(t);
    return (uint32_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
#endif
}

// lt_overlay_text / lt_text_blend_host: white over the frame
IA_HD uint32_t text_over(uint32_t v, int a) { return v + (uint32_t)(((255 - (int)v) * a + 127) / 255); }

// one pixel, R | G << 8 | B << 16: the lane (its remapped value, 0: none), then the text (its glyph's alpha, 0: none)
IA_HD uint32_t draw_pixel(uint32_t px, int lane, int ta, float alpha) {
    uint32_t r = px & 255u, g = (px >> 8) & 255u, b = (px >> 16) & 255u;
    if (lane) g = blend_green(g, lane, alpha);
    if (ta) {
        r = text_over(r, ta);
        g = text_over(g, ta);
        b = text_over(b, ta);
    }
    return r | (g << 8) | (b << 16);
}

// A 2 x 2 block of a 4:2:0 surface: y[0] top left, y[1] top right, y[2] bottom left, y[3] bottom right; one (u, v).
struct Block {
    uint32_t y[4];
    uint32_t u, v;
};
// Draws on the block; -> which of its six bytes changed owner: bit i (0..3) = y[i] was replaced, bit 4 = (u, v) were replaced.
IA_HD unsigned draw_block(Block& b, const int lane[4], const int ta[4], float alpha, const YuvCoef& kin, const sa::Rgb2Yuv& kout) {
    const ya::Chroma c = ya::yuv_chroma((int)b.u, (int)b.v, kin);
    unsigned changed = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        const uint32_t px = ya::yuv_pixel((int)b.y[i], c, kin);
        const uint32_t q = draw_pixel(px, lane[i], ta[i], alpha);
        if (q == px) continue;
        const int r = (int)(q & 255u), g = (int)((q >> 8) & 255u), bl = (int)((q >> 16) & 255u);
        b.y[i] = sa::luma(r, g, bl, kout);
        changed |= 1u << i;
        if (i == 0) {
            b.u = sa::chroma_u(r, g, bl, kout);
            b.v = sa::chroma_v(r, g, bl, kout);
            changed |= 16u;
        }
    }
    return changed;
}

}  // namespace ia
}  // namespace lt
