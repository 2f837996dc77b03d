// Host build of lane_tracker_amd/csrc/inplace_arith.h (with yuv_arith.h and sink_arith.h) for tests/test_inplace_cpu.py: the
// expressions k_inplace.hip runs on a 2 x 2 block of a 4:2:0 surface, compiled with the system C++ compiler and called through ctypes.
#include <cstddef>
#include <cstdint>

#include "inplace_arith.h"

using namespace lt;

extern "C" {

// n blocks: y4 (n x 4: top left, top right, bottom left, bottom right), u, v (n), the lane's value and the glyph's alpha per pixel
// (n x 4, 0: none) -> the blocks after the draw and, per block, which bytes were replaced (bit i: y[i], bit 4: u and v)
void ia_draw_blocks(const uint8_t* y4, const uint8_t* u, const uint8_t* v, const int32_t* lane4, const int32_t* alpha4, size_t n, float alpha,
                    const int32_t* kin5, const int32_t* kout8, uint8_t* y4_out, uint8_t* u_out, uint8_t* v_out, uint8_t* changed) {
    const YuvCoef kin{kin5[0], kin5[1], kin5[2], kin5[3], kin5[4]};
    const sa::Rgb2Yuv kout = sa::coef_of(kout8);
    for (size_t i = 0; i < n; ++i) {
        ia::Block b{{y4[4 * i], y4[4 * i + 1], y4[4 * i + 2], y4[4 * i + 3]}, u[i], v[i]};
        const int lane[4] = {lane4[4 * i], lane4[4 * i + 1], lane4[4 * i + 2], lane4[4 * i + 3]};
        const int ta[4] = {alpha4[4 * i], alpha4[4 * i + 1], alpha4[4 * i + 2], alpha4[4 * i + 3]};
        changed[i] = (uint8_t)ia::draw_block(b, lane, ta, alpha, kin, kout);
        for (int k = 0; k < 4; ++k) y4_out[4 * i + k] = (uint8_t)b.y[k];
        u_out[i] = (uint8_t)b.u;
        v_out[i] = (uint8_t)b.v;
    }
}

// n RGB pixels (R | G << 8 | B << 16) through the lane's and the text's blend
void ia_draw_pixels(const uint32_t* px, const int32_t* lane, const int32_t* ta, size_t n, float alpha, uint32_t* out) {
    for (size_t i = 0; i < n; ++i) out[i] = ia::draw_pixel(px[i], lane[i], ta[i], alpha);
}

}  // extern "C"
