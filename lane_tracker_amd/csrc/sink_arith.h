// The device sinks' per-pixel arithmetic -- RGB -> YUV 4:2:0 in OpenCV's 20-bit fixed point (cv2.cvtColor(img, COLOR_RGB2YUV_I420))
// -- as plain inline functions without HIP types: k_sink.hip runs exactly these expressions on the device, and a host translation
// unit (tests/sink_arith_host.cpp) compiles the same header with the system compiler, so the CPU tests check what the GPU runs.
//
//     Y = clamp((CRY r + CGY g + CBY b + 2^19 + (16  << 20)) >> 20)     every pixel
//     U = clamp((CRU r + CGU g + CBU b + 2^19 + (128 << 20)) >> 20)     the pixel at (even row, even column) of each 2 x 2 block
//     V = clamp((CBU r + CGV g + CBV b + 2^19 + (128 << 20)) >> 20)     the same pixel; its R coefficient IS CBU
//
// coeffs = {CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV}.  The products are 24 x 8 bit (one v_mul_i32_i24 each: every magnitude is
// below 2^23, coeffs_ok) and the clamp comes BEFORE the shift: clamp(v, 0, 2^28 - 1) >> 20 is the same byte as
// clamp(v >> 20, 0, 255), and the shift-then-clamp form has been selected as v_ashr_pk_u8_i32, which tests/test_isa_guards.py
// keeps out of the product.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SA_HD inline
#endif

namespace lt {
namespace sa {

struct Rgb2Yuv {
    int32_t cry, cgy, cby, cru, cgu, cbu, cgv, cbv;
};
SA_HD Rgb2Yuv coef_of(const int32_t* k) { return Rgb2Yuv{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]}; }

// video range; BT601: OpenCV's constants (R2Y .. B2VI of its color_yuv code), BT709: round(c * 2^20) of the BT.709 matrix
// (Kr = 0.2126, Kb = 0.0722; luma scaled by 219 / 255, chroma by 224 / 255)
constexpr int32_t BT601[8] = {269484, 528482, 102760, -155188, -305135, 460324, -385875, -74448};
constexpr int32_t BT709[8] = {191455, 644067, 65019, -105533, -355018, 460551, -418321, -42230};

// A matrix is taken when every product is one 24-bit multiply and no row can leave int32 (the rule of lt_set_input_format):
// every magnitude below 2^23, and sum |c| * 255 + 2^19 + (128 << 20) inside int32 for each of the three rows.
inline bool coeffs_ok(const int32_t* k) {
    auto mag = [](int32_t v) { return v < 0 ? -(long long)v : (long long)v; };
    for (int i = 0; i < 8; ++i)
        if (mag(k[i]) >= (1LL << 23)) return false;
    const long long rows[3] = {mag(k[0]) + mag(k[1]) + mag(k[2]), mag(k[3]) + mag(k[4]) + mag(k[5]), mag(k[5]) + mag(k[6]) + mag(k[7])};
    for (long long s : rows)
        if (s * 255 + (1LL << 19) + (128LL << 20) > 0x7fffffffLL) return false;
    return true;
}

SA_HD int32_t mul24(int32_t c, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(c, v);
#else
    return c * v;
#endif
}
// clamp(v, 0, 2^28 - 1) >> 20: the byte
SA_HD uint32_t byte_of(int32_t v) {
    const int32_t hi = (1 << 28) - 1;
    const int32_t c = v < 0 ? 0 : (v > hi ? hi : v);
    return (uint32_t)c >> 20;
}
SA_HD uint32_t luma(int32_t r, int32_t g, int32_t b, const Rgb2Yuv& k) {
    return byte_of(mul24(k.cry, r) + mul24(k.cgy, g) + mul24(k.cby, b) + ((1 << 19) + (16 << 20)));
}
SA_HD uint32_t chroma_u(int32_t r, int32_t g, int32_t b, const Rgb2Yuv& k) {
    return byte_of(mul24(k.cru, r) + mul24(k.cgu, g) + mul24(k.cbu, b) + ((1 << 19) + (128 << 20)));
}
SA_HD uint32_t chroma_v(int32_t r, int32_t g, int32_t b, const Rgb2Yuv& k) {
    return byte_of(mul24(k.cbu, r) + mul24(k.cgv, g) + mul24(k.cbv, b) + ((1 << 19) + (128 << 20)));
}

}  // namespace sa
}  // namespace lt
