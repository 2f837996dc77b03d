// The front end's per-pixel arithmetic -- the bilinear blend of four RGBX taps and the Lab-b tail -- as plain inline
// functions without HIP types: k_frontend.hip runs exactly these expressions on the device, and a host translation unit
// (tests/front_arith_host.cpp) compiles the same header with the system compiler, so the CPU tests check what the GPU runs.
//
// Why fp32 (profiles/front_f32_valu_issue.txt): on gfx950 v_fma_f32 / v_mul_f32 / v_add_f32 issue in ~2.3 cycles per wave64
// instruction, v_mad_u32_u24 / v_mul_u32_u24 and every byte extract (v_perm_b32, v_bfe_u32, SDWA) in ~4.2.  The blend
//     (sum_i w_i p_i + 512) >> 10,    p_i <= 255,  w_i <= 1024,  sum_i w_i <= 1024
// is  trunc(0.5 + sum_i p_i (w_i / 1024))  and that is EXACT in fp32: every product has at most 19 significant bits, every
// partial sum is a multiple of 2^-10 below 256.5, both fit the 24-bit significand, so no operation rounds (fused or not).
// The functions below return the blend times 8 (weights w_i / 128, start 4.0: multiples of 2^-7 below 2052): the truncated
// value masked with 0x7f8 is the byte offset of the pixel's entry in a table of 8-byte rows, without a shift.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FA_HD inline
#endif

namespace lt {
namespace fa {

// The four tap weights of a pixel, times 8 / 1024: products of the 5-bit fractions (fx, fy in 0..31).  `m` = the taps that lie
// inside the frame, bit 0: top left, 1: top right, 2: bottom left, 3: bottom right; a tap outside gets weight 0 (the constant
// border 0 of the remap), which is the same integer as masking the tap.
struct Weights { float w00, w01, w10, w11; };
FA_HD Weights weights8(int fx, int fy, unsigned m = 15u) {
    const int gx = 32 - fx, gy = 32 - fy;
    constexpr float S = 1.f / 128.f;
    return Weights{(m & 1u) ? (float)(gx * gy) * S : 0.f, (m & 2u) ? (float)(fx * gy) * S : 0.f,
                   (m & 4u) ? (float)(gx * fy) * S : 0.f, (m & 8u) ? (float)(fx * fy) * S : 0.f};
}

// Channel CH (0..2) of four RGBX taps -> floor(8 * (blend + 0.5)): bits 3..10 are the 8-bit result, bits 0..2 are fraction.
// (float)((t >> 8 CH) & 255) is one v_cvt_f32_ubyteN; the chain is four v_fma_f32 / v_fmac_f32 and one v_cvt_u32_f32.
template <int CH>
FA_HD uint32_t blend8(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11, const Weights& w) {
    float s = __builtin_fmaf((float)((t00 >> (8 * CH)) & 255u), w.w00, 4.0f);
    s = __builtin_fmaf((float)((t01 >> (8 * CH)) & 255u), w.w01, s);
    s = __builtin_fmaf((float)((t10 >> (8 * CH)) & 255u), w.w10, s);
    s = __builtin_fmaf((float)((t11 >> (8 * CH)) & 255u), w.w11, s);
    return (uint32_t)s;   // truncates; 0 <= s < 2052
}
// The same value in 24-bit integer multiplies: ((sum_i w_i p_i + 2^9) >> 7.  The weights are masked to 11 bits on purpose: unless
// the compiler can see that they are small it multiplies with v_mul_lo_u32 (quarter rate) instead of v_mul_u32_u24, whose SDWA
// form selects the tap's byte in the multiply itself -- extract and multiply in one 4-cycle instruction, where the fp32 form
// pays a 4-cycle v_cvt_f32_ubyteN and a 2-cycle v_fma_f32.
struct WeightsI { uint32_t top, bot; };   // w00 | w01 << 16, w10 | w11 << 16: the multiply selects the half as it selects the byte
FA_HD WeightsI weights_i(int fx, int fy, unsigned m = 15u) {
    const uint32_t gx = 32u - (uint32_t)fx, gy = 32u - (uint32_t)fy, ux = (uint32_t)fx, uy = (uint32_t)fy;
    const uint32_t w00 = (m & 1u) ? (gx * gy) & 0x7ffu : 0u, w01 = (m & 2u) ? (ux * gy) & 0x7ffu : 0u;
    const uint32_t w10 = (m & 4u) ? (gx * uy) & 0x7ffu : 0u, w11 = (m & 8u) ? (ux * uy) & 0x7ffu : 0u;
    return WeightsI{w00 | (w01 << 16), w10 | (w11 << 16)};
}
template <int CH>
FA_HD uint32_t blend8(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11, const WeightsI& w) {
    return (((t00 >> (8 * CH)) & 255u) * (w.top & 0xffffu) + ((t01 >> (8 * CH)) & 255u) * (w.top >> 16) +
            ((t10 >> (8 * CH)) & 255u) * (w.bot & 0xffffu) + ((t11 >> (8 * CH)) & 255u) * (w.bot >> 16) + 512u) >> 7;
}
constexpr uint32_t ROW8_MASK = 0x7f8u;   // blend8() & ROW8_MASK == 8 * the blended value
FA_HD uint32_t value_of(uint32_t b8) { return b8 >> 3; }

// ---- Lab b ------------------------------------------------------------------------------------------------------------------
// OpenCV's 8-bit RGB2Lab (gamma_shift 3, lab_shift 12, lab_shift2 15).  The gamma table and the Y / Z rows of the matrix are
// folded into one table of 8-byte rows per channel: yz[ch][v] = gamma[v] * (C[3 + ch], C[6 + ch]), the rounding constant 2^11
// of the descale added to the red rows, so that iy = (yz[0][r].y + yz[1][g].y + yz[2][b].y) >> 12 (sums below 2^24).
struct alignas(8) YZ { uint32_t y, z; };
FA_HD YZ yz_row(uint32_t gamma_v, const int32_t* C, int ch) {
    const uint32_t rnd = ch == 0 ? 2048u : 0u;
    return YZ{gamma_v * (uint32_t)C[3 + ch] + rnd, gamma_v * (uint32_t)C[6 + ch] + rnd};
}

// iy / iz index the 3072-entry cube-root table and are clamped to 3071.  The clamp is dead when no row sum can reach 3072:
// with gamma values <= gamma_max and non-negative coefficients, iy <= (gamma_max * (C3 + C4 + C5) + 2^11) >> 12.
FA_HD bool lab_clamp_is_dead(int gamma_max, const int32_t* C) {
    for (int r = 1; r < 3; ++r) {
        long long sum = 0;
        for (int c = 0; c < 3; ++c) {
            if (C[3 * r + c] < 0) return false;
            sum += C[3 * r + c];
        }
        if (((long long)gamma_max * sum + 2048) >> 12 > 3071) return false;
    }
    return true;
}

// byte offset of cbrt_tab[min(sum >> 12, 3071)]; CLAMP = false: (sum >> 11) & ~1, one shift and one AND of the 2-cycle class
template <bool CLAMP>
FA_HD uint32_t cbrt_offset(uint32_t sum) {
    if (CLAMP) {
        const uint32_t i = sum >> 12;
        return (i > 3071u ? 3071u : i) * 2u;
    }
    return (sum >> 11) & 0x1ffeu;
}

// b = clamp((200 (fY - fZ) + 128 * 2^15 + 2^14) >> 15, 0, 255)
FA_HD int lab_b_value(int fY, int fZ) {
    const int v = (200 * (fY - fZ) + 128 * (1 << 15) + (1 << 14)) >> 15;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// The whole tail from the three table rows of a pixel (what k_warp_split4 does with its LDS copies of the tables).
template <bool CLAMP>
FA_HD int lab_b_rows(const YZ& r, const YZ& g, const YZ& b, const uint16_t* cbrt_tab) {
    const uint32_t oy = cbrt_offset<CLAMP>(r.y + g.y + b.y), oz = cbrt_offset<CLAMP>(r.z + g.z + b.z);
    const int fY = *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(cbrt_tab) + oy);
    const int fZ = *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(cbrt_tab) + oz);
    return lab_b_value(fY, fZ);
}

}  // namespace fa
}  // namespace lt
