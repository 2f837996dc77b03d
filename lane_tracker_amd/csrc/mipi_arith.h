// MIPI-packed RAW10 / RAW12 Bayer rows (CSI-2; V4L2 SRGGB10P / SRGGB12P and their siblings) -- where the samples of a run of sites lie
// and how they come out of the bytes -- as plain inline functions without HIP types: k_frontend.hip (the walk's window rows, the row
// conversion) runs exactly these expressions on the device, and a host program (tests/raw_packed_host.cpp) compiles the same header with
// the system compiler, so the CPU tests check what the GPU runs.  What comes out is the 16-bit word of the unpacked layouts, so that
// everything behind the mosaic (shading, raw table, demosaic, colour stage: shade_arith.h, bayer_arith.h) is what it is for those.
//
//   RAW10 (PACK10): W % 4 == 0, a row is 5 W / 4 bytes.  Group g holds sites 4g .. 4g + 3: byte 5g + i is s[4g + i] >> 2 (i = 0 .. 3) and
//                   bits 2i + 1 : 2i of byte 5g + 4 are s[4g + i] & 3.
//   RAW12 (PACK12): W even, a row is 3 W / 2 bytes.  Byte 3g is s[2g] >> 4, byte 3g + 1 is s[2g + 1] >> 4, byte 3g + 2 is
//                   (s[2g] & 15) | (s[2g + 1] & 15) << 4.
// No bits lie above a sample: nothing is masked or ignored.
//
// The walk's window: the four sites bx .. bx + 3 of a row (bx <= W - 4) need the bytes from first_byte(bx) on -- at most 9 (RAW10) or 8
// (RAW12) of them, whatever bx: they lie inside the three aligned dwords that hold the 8 + 3 bytes from any byte address, the 96-bit load
// of the 16-bit walk.  Where the high byte and the low bits of each of the four sites lie inside that window depends on bx alone, not on
// the frame: unpack_of(bx) turns it into four byte selectors and two pairs of shifts once per walk, and samples4 applies them to the
// window's dwords -- per pair of sites two byte permutes, one packed 16-bit shift, a mask and a shift-or; no multiply, no memory access.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MA_HD inline
#endif

namespace lt {
namespace ma {

constexpr int PACK10 = 0, PACK12 = 1;        // (-1 where a packing is optional: none, 16-bit words)
MA_HD constexpr int bits_of(int pack) { return pack == PACK10 ? 10 : 12; }
// the bytes of a row of w sites (w % 4 == 0 / w even), and the byte that holds the high bits of site x: 5 (x >> 2) + (x & 3) = x + (x >> 2),
// 3 (x >> 1) + (x & 1) = x + (x >> 1) -- shifts and adds
MA_HD constexpr int row_bytes(int pack, int w) { return pack == PACK10 ? w + (w >> 2) : w + (w >> 1); }
MA_HD constexpr int high_byte(int pack, int x) { return pack == PACK10 ? x + (x >> 2) : x + (x >> 1); }
// ... the byte that holds its low bits, and the bit they start at
MA_HD constexpr int low_byte(int pack, int x) { return pack == PACK10 ? high_byte(pack, x | 3) + 1 : high_byte(pack, x | 1) + 1; }
MA_HD constexpr int low_shift(int pack, int x) { return pack == PACK10 ? 2 * (x & 3) : 4 * (x & 1); }
// the first byte that the window of the four sites from bx needs: the high byte of site bx
MA_HD constexpr int first_byte(int pack, int bx) { return high_byte(pack, bx); }

// one site of a row, byte accesses (the site-wise body of the row conversion; the definition the tests restate)
MA_HD uint32_t site_at(int pack, const uint8_t* row, int x) {
    const uint32_t h = row[high_byte(pack, x)], l = row[low_byte(pack, x)];
    return pack == PACK10 ? (h << 2) | ((l >> low_shift(pack, x)) & 3u) : (h << 4) | ((l >> low_shift(pack, x)) & 15u);
}

// ---- the two instructions the extraction is made of, as the device has them (v_perm_b32, v_pk_lshrrev_b16) --------------------------
// byte j of the result: byte sel[j] of the eight bytes {hi, lo} (0 .. 3: lo, 4 .. 7: hi), or 0 where sel[j] is 0x0c
MA_HD uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int j = 0; j < 4; ++j) {
        const uint32_t s = (sel >> (8 * j)) & 255u;
        if (s < 8) out |= (uint32_t)((v >> (8 * s)) & 255u) << (8 * j);
    }
    return out;
#endif
}
// each 16-bit half of v shifted right by the same half of sh (0 .. 15)
MA_HD uint32_t pk_shr16(uint32_t v, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, v) >> __builtin_bit_cast(u16x2, sh));
#else
    return ((v & 0xffffu) >> (sh & 15u)) | (((v >> 16) >> ((sh >> 16) & 15u)) << 16);
#endif
}

// ---- the window of the walk ---------------------------------------------------------------------------------------------------
// Where site bx + k (k = 0 .. 3) lies in the window that starts at first_byte(bx): the byte of its high bits, the byte of its low bits
// (both relative to the window's first byte) and the bit its low bits start at.  i = bx & 3 (RAW10) / bx & 1 (RAW12).
struct Site { int hpos, lpos, sh; };
MA_HD Site site_of(int pack, int i, int k) {
    const int j = i + k;
    if (pack == PACK10) return j < 4 ? Site{k, 4 - i, 2 * j} : Site{k + 1, 9 - i, 2 * (j - 4)};
    const int p = j >> 1, q = j & 1;
    return Site{3 * p + q - i, 3 * p + 2 - i, 4 * q};
}
// What turns the window's dwords w0 (bytes 0 .. 3), w1 (4 .. 7), w2 (8 .. 11) into the four samples: per pair of sites (sites 0, 1: lo;
// sites 2, 3: hi) the selector of their high bytes, the selector of the bytes with their low bits -- each into bytes 0 and 2 of a
// dword, bytes 1 and 3 zero -- and the shifts of the two.  Every position is below 8, in {w1, w0}, but one: RAW10 with bx & 3 == 1 has
// the low bits of site 3 in byte 8, and those of site 2 in byte 3 -- `far`: that one permute takes {w2, w0}.  (RAW12 never reads w2.)
struct Unpack { uint32_t hlo, hhi, llo, lhi, slo, shi; bool far; };
MA_HD uint32_t sel2(int a, int b) { return (uint32_t)a | 0x0c00u | ((uint32_t)b << 16) | 0x0c000000u; }
MA_HD Unpack unpack_of(int pack, int bx) {
    const int i = pack == PACK10 ? bx & 3 : bx & 1;
    const Site s0 = site_of(pack, i, 0), s1 = site_of(pack, i, 1), s2 = site_of(pack, i, 2), s3 = site_of(pack, i, 3);
    const bool far = pack == PACK10 && i == 1;
    const int l2 = s2.lpos, l3 = far ? s3.lpos - 4 : s3.lpos;          // (byte 8 is byte 0 of w2, selector 4 of {w2, w0})
    return Unpack{sel2(s0.hpos, s1.hpos), sel2(s2.hpos, s3.hpos), sel2(s0.lpos, s1.lpos), sel2(l2, l3),
                  (uint32_t)s0.sh | ((uint32_t)s1.sh << 16), (uint32_t)s2.sh | ((uint32_t)s3.sh << 16), far};
}
// the four samples as the 16-bit layouts hold them: lo = s[bx] | s[bx + 1] << 16, hi = s[bx + 2] | s[bx + 3] << 16
template <int PACK>
MA_HD void samples4(const Unpack& u, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t& lo, uint32_t& hi) {
    constexpr int K = PACK == PACK10 ? 2 : 4;
    constexpr uint32_t M = PACK == PACK10 ? 0x00030003u : 0x000f000fu;
    const uint32_t wf = PACK == PACK10 && u.far ? w2 : w1;
    lo = (perm(w1, w0, u.hlo) << K) | (pk_shr16(perm(w1, w0, u.llo), u.slo) & M);
    hi = (perm(w1, w0, u.hhi) << K) | (pk_shr16(perm(wf, w0, u.lhi), u.shi) & M);
}

// ---- the 16 columns of the row conversion's wide body -----------------------------------------------------------------------------
// 16 sites from a column that is a multiple of 16 are 20 / 24 bytes from a byte that is a multiple of 4 -- five / six dwords `m` -- and
// the four sites 4j .. 4j + 3 of them (j = 0 .. 3) lie at constant positions: every shift below is an immediate.
MA_HD uint32_t byte_of(const uint32_t* m, int pos) { return (m[pos >> 2] >> (8 * (pos & 3))) & 255u; }
template <int PACK>
MA_HD void group4(const uint32_t* m, int j, uint32_t& lo, uint32_t& hi) {
    if (PACK == PACK10) {
        const int b = 5 * j;
        const uint32_t l = byte_of(m, b + 4);
        lo = ((byte_of(m, b) << 2) | (l & 3u)) | (((byte_of(m, b + 1) << 2) | ((l >> 2) & 3u)) << 16);
        hi = ((byte_of(m, b + 2) << 2) | ((l >> 4) & 3u)) | (((byte_of(m, b + 3) << 2) | (l >> 6)) << 16);
    } else {
        const int b = 6 * j;
        const uint32_t la = byte_of(m, b + 2), lb = byte_of(m, b + 5);
        lo = ((byte_of(m, b) << 4) | (la & 15u)) | (((byte_of(m, b + 1) << 4) | (la >> 4)) << 16);
        hi = ((byte_of(m, b + 3) << 4) | (lb & 15u)) | (((byte_of(m, b + 4) << 4) | (lb >> 4)) << 16);
    }
}

}  // namespace ma
}  // namespace lt
