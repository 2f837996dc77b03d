// Lens-shading correction of raw Bayer input (lt_set_raw_shading) -- the gain that depends on the position in the image -- as plain inline
// functions without HIP types: k_frontend.hip (the expansion of the mesh, the walks, the row conversion) runs exactly these expressions
// on the device, and a host program (tests/raw_shading_host.cpp) compiles the same header with the system compiler, so the CPU tests check
// what the GPU runs.  Shading comes first: shading, raw table, demosaic, colour stage (bayer_arith.h holds the other three).
//
// The map is a mesh uint16[4][mh][mw] of gains in Q12 (4096 is 1.0; any uint16 is legal), phase-major as a raw table is (bayer_arith.h:
// phase), 2 <= mw, mh <= 64, node (0, 0) on pixel (0, 0) and node (mh - 1, mw - 1) on pixel (H - 1, W - 1).  The gain of site (y, x):
//     u = x (mw - 1) 256 / (W - 1);  j = min(u >> 8, mw - 2);  a = u - (j << 8)          (0 .. 256; integer division)
//     v = y (mh - 1) 256 / (H - 1);  i = min(v >> 8, mh - 2);  b = v - (i << 8)
//     G = ((256 - a)(256 - b) m[p][i][j] + a (256 - b) m[p][i][j + 1] + (256 - a) b m[p][i + 1][j] + a b m[p][i + 1][j + 1] + 32768) >> 16
// in unsigned 32-bit arithmetic (the weights sum to 65536: the sum stays below 2^32), p the site's phase.  A sample s (the byte, or the
// word masked to `bits`) with the pedestal B = black[p], 0 <= B <= smax (255 or (1 << bits) - 1), becomes
//     s' = min(max(B + (((s - B) G + 2048) >> 12), 0), smax)                              int32, arithmetic shift (floor)
// |s - B| <= 4095 and G <= 65535: every product is an exact 24-bit multiply and stays below 2^31.  G = 4096 is the identity.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SA_HD inline
#endif

namespace lt {
namespace sa {

constexpr int MESH_MIN = 2, MESH_MAX = 64;

// One axis of the expansion: coordinate c of n samples under a mesh of m nodes -> the node in front of it and the weight (0 .. 256) of the next one.
struct Node { uint32_t i, w; };
SA_HD Node node_of(int c, int n, int m) {
    const uint32_t u = (uint32_t)c * (uint32_t)(m - 1) * 256u / (uint32_t)(n - 1);       // (c <= 16383, m - 1 <= 63: below 2^28)
    const uint32_t i = (u >> 8) < (uint32_t)(m - 2) ? (u >> 8) : (uint32_t)(m - 2);
    return Node{i, u - (i << 8)};
}
// The gain of site (y, x) of an h x w image from the mesh plane of its phase (mh rows of mw nodes).
SA_HD uint32_t gain_at(const uint16_t* m, int mw, int mh, int y, int x, int h, int w) {
    const Node nx = node_of(x, w, mw), ny = node_of(y, h, mh);
    const uint16_t* r0 = m + ny.i * (uint32_t)mw + nx.i;
    const uint16_t* r1 = r0 + mw;
    const uint32_t a = nx.w, b = ny.w;
    return ((256u - a) * (256u - b) * r0[0] + a * (256u - b) * r0[1] + (256u - a) * b * r1[0] + a * b * r1[1] + 32768u) >> 16;
}

// What a walk keeps of a pedestal B: B itself and the rounding term of the sample's expression with B folded in -- B + (t >> 12) ==
// (t + (B << 12)) >> 12 for every int t, so the add behind the shift costs nothing (4095 * 65535 + 2048 + (4095 << 12) < 2^31).
SA_HD int round_term(int black) { return (black << 12) + 2048; }
// difference (|d| <= 4095) times gain (<= 65535): on the device a 24-bit multiply, which is what it is
SA_HD int mul24g(int d, int gain) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(d, gain);
#else
    return d * gain;
#endif
}
// One sample: s (already masked to the sample's bits), its pedestal, round_term(pedestal), its gain, smax.
SA_HD uint32_t shade(uint32_t s, int black, int rterm, uint32_t gain, int smax) {
    const int v = (mul24g((int)s - black, (int)gain) + rterm) >> 12;
    const int lo = v < 0 ? 0 : v;            // (a max, then a min: with a constant smax one median of three, with a run-time one two instructions)
    return (uint32_t)(lo > smax ? smax : lo);
}
// ... as the definition writes it (the tests hold the two against each other)
SA_HD uint32_t shade_plain(uint32_t s, int black, uint32_t gain, int smax) {
    const int v = black + ((((int)s - black) * (int)gain + 2048) >> 12);
    return (uint32_t)(v < 0 ? 0 : (v > smax ? smax : v));
}

// The pedestals of the two sites that alternate along a row of the mosaic, as the kernels hold them.
struct Black2 { int ba, ra, bb, rb; };       // site 0, 2, ..: ba and its round term; site 1, 3, ..: bb
SA_HD Black2 black2(int black_a, int black_b) { return Black2{black_a, round_term(black_a), black_b, round_term(black_b)}; }

// bayer_arith.h's condition4 with the shading between a byte's extraction and its lookup: the four bytes of dword w -- consecutive sites of
// one row, byte 0 the first -- with their gains (glo: sites 0, 1 in its low / high half; ghi: sites 2, 3), shaded, then looked up in the
// table rows rowa (sites 0, 2) / rowb (sites 1, 3).
SA_HD uint32_t shade_condition4(uint32_t w, uint32_t glo, uint32_t ghi, const Black2& k, const uint8_t* rowa, const uint8_t* rowb) {
    return (uint32_t)rowa[shade(w & 255u, k.ba, k.ra, glo & 0xffffu, 255)] | ((uint32_t)rowb[shade((w >> 8) & 255u, k.bb, k.rb, glo >> 16, 255)] << 8) |
           ((uint32_t)rowa[shade((w >> 16) & 255u, k.ba, k.ra, ghi & 0xffffu, 255)] << 16) | ((uint32_t)rowb[shade(w >> 24, k.bb, k.rb, ghi >> 16, 255)] << 24);
}
// ... and condition4w: the four 16-bit sites that the dwords lo (sites 0, 1) and hi (sites 2, 3) hold, mask = (1 << bits) - 1 = smax.
SA_HD uint32_t shade_condition4w(uint32_t lo, uint32_t hi, uint32_t glo, uint32_t ghi, const Black2& k, const uint8_t* rowa, const uint8_t* rowb,
                                 uint32_t mask) {
    return (uint32_t)rowa[shade(lo & mask, k.ba, k.ra, glo & 0xffffu, (int)mask)] | ((uint32_t)rowb[shade((lo >> 16) & mask, k.bb, k.rb, glo >> 16, (int)mask)] << 8) |
           ((uint32_t)rowa[shade(hi & mask, k.ba, k.ra, ghi & 0xffffu, (int)mask)] << 16) |
           ((uint32_t)rowb[shade((hi >> 16) & mask, k.bb, k.rb, ghi >> 16, (int)mask)] << 24);
}

}  // namespace sa
}  // namespace lt
