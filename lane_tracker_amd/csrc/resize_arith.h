// cv2.resize(frame, dsize) with the default INTER_LINEAR on u8 -- half-pixel centres, 11-bit coefficients, OpenCV's two-stage
// fixed-point rounding -- as plain inline functions without HIP types: the arithmetic utils.resize_linear and oracle.resize_linear
// restate.  lt_api.cpp builds the tap tables of a context's input size with resize_tap, k_resize.hip blends with resize_blend, and
// a host translation unit (tests/resize_arith_host.cpp) compiles the same header with the system compiler, so the CPU tests check
// what the GPU runs.
//
// Every product has factors below 2^24 -- a sample times a coefficient is at most 255 * 2048, a coefficient times a shifted row sum
// at most 2048 * 32640 -- so each is one 24-bit multiply (v_mul_u32_u24 / v_mad_u32_u24) whose low 32 bits are the exact product.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RZ_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RZ_HD inline
#endif

namespace lt {
namespace rz {

constexpr int SIZE_MAX_AXIS = 16384;     // the largest width / height of an input frame (lt_set_input_size)

// The two taps of destination index i along an axis of src_len -> dst_len samples and their coefficients, in the operations of
// utils._resize_taps: the f64 product cast to f32, the floor, both clamps with the fraction zeroed, rint(f * 2048) for each
// coefficient.  tap1 is tap0 + 1, or tap0 where the last sample is clamped (its coefficient is 0 there).
struct Tap { int32_t tap0, tap1, c0, c1; };
inline Tap resize_tap(int src_len, int dst_len, int i) {
    const double scale = (double)src_len / (double)dst_len;
    float f = (float)(((double)i + 0.5) * scale - 0.5);
    const float fl = std::floor(f);
    long long s = (long long)fl;
    f = f - fl;
    if (s < 0) { s = 0; f = 0.f; }
    else if (s >= src_len - 1) { s = src_len - 1; f = 0.f; }
    const float c1 = std::nearbyint(f * 2048.f), c0 = std::nearbyint((1.f - f) * 2048.f);
    return Tap{(int32_t)s, (int32_t)(s + 1 < src_len - 1 ? s + 1 : src_len - 1), (int32_t)c0, (int32_t)c1};
}

// The source samples [*s0, *s1) that destination samples [a, b) read: taps are monotone along an axis, so the first sample's upper
// tap and the last sample's lower tap bound them.  Empty for an empty run.
inline void input_run(int src_len, int dst_len, int a, int b, int* s0, int* s1) {
    if (b <= a) { *s0 = *s1 = 0; return; }
    *s0 = resize_tap(src_len, dst_len, a).tap0;
    *s1 = resize_tap(src_len, dst_len, b - 1).tap1 + 1;
}

RZ_HD uint32_t mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}

// One channel: the samples of the upper tap row (p00, p01) and the lower one (p10, p11) at the two horizontal taps, the horizontal
// coefficients (a0, a1) and the vertical ones (b0, b1) -> the output sample.  Coefficient pairs sum to 2048: the result is <= 255.
RZ_HD uint32_t resize_blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
    const uint32_t h0 = mul24(p00, a0) + mul24(p01, a1), h1 = mul24(p10, a0) + mul24(p11, a1);
    return ((mul24(b0, h0 >> 4) >> 16) + (mul24(b1, h1 >> 4) >> 16) + 2u) >> 2;
}

// A destination column as the kernel reads it, two words: where the 8-byte window of a tap row starts -- byte 3 * xl of the row, xl =
// min(tap0, src_w - 2) clamped at 0, so that both taps lie inside it and it starts inside the row -- which of its two pixels each
// tap is, and the coefficients.
//   word 0: 3 * xl | (tap0 - xl) << 16 | (tap1 - xl) << 17        word 1: c0 | c1 << 16
inline void pack_column(const Tap& t, int src_w, uint32_t out[2]) {
    const int xl = t.tap0 < src_w - 2 ? t.tap0 : (src_w - 2 > 0 ? src_w - 2 : 0);
    out[0] = (uint32_t)(3 * xl) | ((uint32_t)(t.tap0 - xl) << 16) | ((uint32_t)(t.tap1 - xl) << 17);
    out[1] = (uint32_t)t.c0 | ((uint32_t)t.c1 << 16);
}

}  // namespace rz
}  // namespace lt
