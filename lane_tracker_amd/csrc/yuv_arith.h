// The YUV 4:2:0 and packed 4:2:2 inputs' per-pixel arithmetic -- OpenCV's 8-bit YUV -> RGB (cv2.cvtColor(COLOR_YUV2RGB_NV12 / _I420)): 20-bit fixed
// point in int32, one (U, V) pair per 2 x 2 block, no chroma interpolation -- as plain inline functions without HIP types:
// k_frontend.hip (the undistortion's taps, the row conversion) and k_inplace.hip (the blocks a lane or a text line lands on) run
// exactly these expressions on the device, and a host translation unit (tests/inplace_arith_host.cpp) compiles the same header
// with the system compiler, so the CPU tests check what the GPU runs.
//
// The coefficients are below 2^23 in magnitude and the samples are 9-bit, so every product is a v_mul_i32_i24 / v_mad_i32_i24
// whose low 32 bits are the exact product: no quarter-rate multiply and no table.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define YA_HD inline
#endif

namespace lt {

// YUV 4:2:0 input (lt_set_input_format): the five 20-bit fixed-point coefficients of the conversion, each below 2^23 in
// magnitude (checked where they enter), so that every product with a 9-bit sample is one 24-bit multiply
struct YuvCoef {
    int32_t cy, cvr, cvg, cug, cub;
};

namespace ya {

YA_HD int mul24(int c, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(c, v);
#else
    return c * v;
#endif
}

struct Chroma { int r, g, b; };      // the three chroma terms of a (U, V) pair, rounding constant included
YA_HD Chroma yuv_chroma(int u, int v, const YuvCoef& k) {
    u -= 128;
    v -= 128;
    return Chroma{mul24(k.cvr, v) + (1 << 19), mul24(k.cvg, v) + mul24(k.cug, u) + (1 << 19), mul24(k.cub, u) + (1 << 19)};
}
// clamp(v >> 20, 0, 255), written clamp first: "shift right, clamp to 0..255" of two values packed into one word is what hipcc
// turns into v_ashr_pk_u8_i32 (DESIGN.md "Toolchain cases"; tests/test_isa_guards.py), and it did in the row conversion
YA_HD int clamp_sh20(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return min(max(v, 0), (256 << 20) - 1) >> 20;
#else
    const int hi = (256 << 20) - 1;
    return (v < 0 ? 0 : (v > hi ? hi : v)) >> 20;
#endif
}
// -> R | G << 8 | B << 16
YA_HD uint32_t yuv_pixel(int yy, const Chroma& c, const YuvCoef& k) {
    // (cy is positive and below 2^23: the mask says so to the compiler, which otherwise widens this one to v_mul_lo_u32)
#if defined(__HIP_DEVICE_COMPILE__)
    const int y = (int)__umul24((uint32_t)max(yy - 16, 0), (uint32_t)k.cy & 0x7fffffu);
#else
    const int y = (int)((uint32_t)(yy > 16 ? yy - 16 : 0) * ((uint32_t)k.cy & 0x7fffffu));
#endif
    return (uint32_t)clamp_sh20(y + c.r) | ((uint32_t)clamp_sh20(y + c.g) << 8) | ((uint32_t)clamp_sh20(y + c.b) << 16);
}

// ---- packed 4:2:2 (YUY2 / UYVY input) -----------------------------------------------------------------------------------------
// A row of a W-pixel frame is W / 2 macropixels of four bytes -- ORDER 0, YUY2: Y0 U Y1 V; ORDER 1, UYVY: U Y0 V Y1 -- and the
// conversion is yuv_chroma / yuv_pixel above with the macropixel's (U, V) for both of its pixels (cv2.cvtColor(COLOR_YUV2RGB_YUY2 /
// _UYVY)).  What is new is where the bytes lie.  The two taps of a bilinear sample's tap row, columns cxl and cxl + 1 (0 <= cxl <=
// W - 2), lie inside two consecutive macropixels: one 8-byte window of the row, two dwords.  The window starts at macropixel
// min(cxl >> 1, W / 2 - 2): it never starts before the row and never ends behind it (W >= 4), so nothing outside a row's 2 W bytes
// is ever asked for.  A column's samples are then found by picking the dword of its macropixel and shifting -- 32-bit operations.
constexpr int ORDER_YUY2 = 0, ORDER_UYVY = 1;
// first macropixel of the window of taps cxl, cxl + 1; last_mp = W / 2 - 2
YA_HD int win422_mp(int cxl, int last_mp) { const int m = cxl >> 1; return m < last_mp ? m : last_mp; }
// byte column of that window in its row
YA_HD int win422_col(int mp) { return 4 * mp; }
// which dword (0 / 1) of the window that starts at macropixel mp holds column cx
YA_HD int win422_dword(int cx, int mp) { return (cx >> 1) - mp; }
// bit positions of a column's Y and of its macropixel's U and V inside that dword
YA_HD int ysh422(int order, int cx) { return 16 * (cx & 1) + 8 * order; }
YA_HD int ush422(int order) { return order == ORDER_YUY2 ? 8 : 0; }
YA_HD int vsh422(int order) { return order == ORDER_YUY2 ? 24 : 16; }
// one pixel of a macropixel's dword (its Y at bit ysh) -> R | G << 8 | B << 16
YA_HD uint32_t yuv422_pixel(uint32_t mp_dword, int order, int ysh, const YuvCoef& k) {
    const Chroma c = yuv_chroma((int)((mp_dword >> ush422(order)) & 255u), (int)((mp_dword >> vsh422(order)) & 255u), k);
    return yuv_pixel((int)((mp_dword >> ysh) & 255u), c, k);
}

}  // namespace ya
}  // namespace lt
