// The raw Bayer inputs' arithmetic -- 8-bit bilinear demosaic (what cv2.cvtColor(COLOR_BayerRGGB2RGB / GRBG / GBRG / BGGR) is understood
// to compute; no OpenCV was at hand to check that, DESIGN.md 6.y.3 states the definition) -- as plain inline functions without HIP
// types: k_frontend.hip (the undistortion's taps, the row conversion) runs exactly these expressions on the device, and a host
// translation unit (tests/bayer_arith_host.cpp) compiles the same header with the system compiler, so the CPU tests check what the
// GPU runs.  10- and 12-bit frames (16-bit words) reach this arithmetic through their raw table, which yields bytes (tests/
// bayer_wide_host.cpp); what follows the demosaic, the colour stage, is the last section (tests/raw_color_host.cpp).
//
// A frame is one plane of H rows of W bytes, H and W even and at least 4.  The pixel at (y, x) carries the colour at position
// 2 (y & 1) + (x & 1) of the pattern's name.  An interior pixel (1 <= y <= H - 2, 1 <= x <= W - 2) is demosaiced from its 3 x 3
// neighbourhood; a border pixel takes the value of the interior pixel at (clamp(y, 1, H - 2), clamp(x, 1, W - 2)), that pixel's own
// colour phase included.  The demosaic is sums of at most four bytes: no multiply at all.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BA_HD inline
#endif

namespace lt {
namespace ba {

// The patterns in the order of their layouts (LT_INPUT_BAYER_RGGB + PATTERN): RGGB, GRBG, GBRG, BGGR.  What tells them apart is the
// parity (row, column) of the red sites.
constexpr int PATTERN_RGGB = 0, PATTERN_GRBG = 1, PATTERN_GBRG = 2, PATTERN_BGGR = 3;
BA_HD constexpr int red_row(int pattern) { return pattern >> 1; }
BA_HD constexpr int red_col(int pattern) { return pattern & 1; }

// The colour phase of site (y, x): bit 1 set on the rows of blue, bit 0 set on the columns of blue -- 0: a red site, 3: a blue site,
// 1: green on a red row (red left and right, blue above and below), 2: green on a blue row.
BA_HD constexpr int phase(int pattern, int y, int x) { return 2 * ((y ^ red_row(pattern)) & 1) + ((x ^ red_col(pattern)) & 1); }

BA_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// where a tap at coordinate s of an axis of n samples is demosaiced
BA_HD int tap_pos(int s, int n) { return clampi(s, 1, n - 2); }
// A bilinear sample has taps s and s + 1 on each axis.  Their clamped positions and the 3 x 3 neighbourhoods of those lie inside the
// four samples from win_origin(s, n): the window never starts before sample 0 and never ends behind sample n - 1 (n >= 4), and each
// clamped tap sits at offset 1 or 2 inside it.
BA_HD int win_origin(int s, int n) { return clampi(s - 1, 0, n - 4); }
// One axis of a sample as the walk hands it over -- c0, c1: the taps s and s + 1, each clamped to [0, n - 1] (clamping to the frame
// first changes neither the window nor the tap positions) -> the window's first sample, the taps' offsets inside it (1 or 2) and
// the parities of the positions they are demosaiced at.
struct Axis { int origin, o0, o1, par0, par1; };
BA_HD Axis place_axis(int c0, int c1, int n) {
    const int t0 = tap_pos(c0, n), t1 = tap_pos(c1, n), origin = win_origin(c0, n);
    return Axis{origin, t0 - origin, t1 - origin, t0 & 1, t1 & 1};
}
// the phase of a tap from the parities of its row and column
BA_HD constexpr int phase_of(int pattern, int par_y, int par_x) { return 2 * (par_y ^ red_row(pattern)) + (par_x ^ red_col(pattern)); }

// The source rows that the windows of the camera rows [r0, r1) touch (r0 < r1): the run widened by the 3 x 3 support and by the
// window's clamp -- what a partial upload has to bring.
BA_HD void input_run(int r0, int r1, int h, int* s0, int* s1) {
    const int lo = clampi(r0 - 1, 0, h - 4), hi = r1 + 1 > lo + 4 ? r1 + 1 : lo + 4;
    *s0 = lo;
    *s1 = hi < h ? hi : h;
}
// ... and those that the demosaic of camera rows [a, b) reads (a < b)
BA_HD void support_run(int a, int b, int h, int* s0, int* s1) {
    *s0 = tap_pos(a, h) - 1;
    *s1 = tap_pos(b - 1, h) + 2;
}

// One pixel from its neighbourhood: c the site's own sample, hs / vs the sums of its two horizontal / vertical neighbours, ds the sum
// of its four diagonal ones; ph its phase.  -> R | G << 8 | B << 16
BA_HD uint32_t demosaic(uint32_t c, uint32_t hs, uint32_t vs, uint32_t ds, int ph) {
    const bool green = ((ph ^ (ph >> 1)) & 1) != 0, blue_row = (ph & 2) != 0;
    const uint32_t g = green ? c : (hs + vs + 2u) >> 2;
    const uint32_t p = green ? (hs + 1u) >> 1 : c;            // the colour of this row's red / blue sites
    const uint32_t q = green ? (vs + 1u) >> 1 : (ds + 2u) >> 2;   // the other one
    const uint32_t r = blue_row ? q : p, b = blue_row ? p : q;
    return r | (g << 8) | (b << 16);
}

// The tap at offsets (oy, ox), each 1 or 2, of a 4 x 4 window given as its four rows (byte i of a row: column i), with phase ph.
BA_HD uint32_t window_tap(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, int oy, int ox, int ph) {
    const int sh = 8 * (ox - 1);
    const uint32_t up = (oy == 1 ? r0 : r1) >> sh, mid = (oy == 1 ? r1 : r2) >> sh, dn = (oy == 1 ? r2 : r3) >> sh;   // columns ox - 1, ox, ox + 1 in bytes 0, 1, 2
    const uint32_t c = (mid >> 8) & 255u, hs = (mid & 255u) + ((mid >> 16) & 255u);
    const uint32_t vs = ((up >> 8) & 255u) + ((dn >> 8) & 255u);
    const uint32_t ds = (up & 255u) + ((up >> 16) & 255u) + (dn & 255u) + ((dn >> 16) & 255u);
    return demosaic(c, hs, vs, ds, ph);
}

// ---- raw tables (lt_set_raw_lut) -------------------------------------------------------------------------------------------------
// A raw table is uint8[4][256], one row per colour phase: the conditioned mosaic is s'(y, x) = lut[phase(pattern, y, x)][s(y, x)] and
// everything else is the arithmetic above on s'.  Along a row of the mosaic the phase alternates between the two of that row, so a run
// of sites is conditioned with two row bases, that of its first site and that of the next.

// byte offset of the table row of the site with row parity par_y and column parity par_x
BA_HD constexpr int lut_row(int pattern, int par_y, int par_x) { return 256 * phase_of(pattern, par_y, par_x); }
// The four bytes of dword w -- consecutive sites of one row of the mosaic, byte 0 the first -- conditioned: rowa / rowb are the table
// rows (lut + lut_row(..)) of the sites at bytes 0, 2 and at bytes 1, 3.  The one expression of the kernels and the host test.
BA_HD uint32_t condition4(uint32_t w, const uint8_t* rowa, const uint8_t* rowb) {
    return (uint32_t)rowa[w & 255u] | ((uint32_t)rowb[(w >> 8) & 255u] << 8) | ((uint32_t)rowa[(w >> 16) & 255u] << 16) |
           ((uint32_t)rowb[w >> 24] << 24);
}
// one site
BA_HD uint32_t condition1(uint32_t s, const uint8_t* row) { return row[s & 255u]; }

// ---- wide raw tables (lt_set_raw_lut_wide) ------------------------------------------------------------------------------------------
// 10- and 12-bit raw Bayer: a site is the low `bits` bits of a little-endian 16-bit word, the table uint8[4][1 << bits], phase-major, and
// the conditioned mosaic s'(y, x) = lut[phase(pattern, y, x)][s(y, x) & ((1 << bits) - 1)] is 8-bit: everything else is the arithmetic
// above on s'.  The bits of a word above `bits` are ignored: the mask is what keeps every index inside the table.

// byte offset of the table row of the site with row parity par_y and column parity par_x
BA_HD constexpr int lut_row_wide(int bits, int pattern, int par_y, int par_x) { return (1 << bits) * phase_of(pattern, par_y, par_x); }
// The four consecutive sites of one row of the mosaic that the dwords lo (sites 0, 1) and hi (sites 2, 3) hold, conditioned into the
// dword of four bytes that window_tap takes: rowa / rowb are the table rows of sites 0, 2 and of sites 1, 3, mask = (1 << bits) - 1.
BA_HD uint32_t condition4w(uint32_t lo, uint32_t hi, const uint8_t* rowa, const uint8_t* rowb, uint32_t mask) {
    return (uint32_t)rowa[lo & mask] | ((uint32_t)rowb[(lo >> 16) & mask] << 8) | ((uint32_t)rowa[hi & mask] << 16) |
           ((uint32_t)rowb[(hi >> 16) & mask] << 24);
}
// one site (a 16-bit word, or anything that holds it in its low 16 bits)
BA_HD uint32_t condition1w(uint32_t s, const uint8_t* row, uint32_t mask) { return row[s & mask]; }

// ---- the colour stage (lt_set_raw_color) ---------------------------------------------------------------------------------------------
// After the demosaic: a colour-correction matrix m, int16 3 x 3 in Q10 (1024 is 1.0; row c makes output channel c), row-major as nine
// ints, then one 256-entry output curve:
//     v[c]   = (m[3c] * R + m[3c + 1] * G + m[3c + 2] * B + 512) >> 10         int32, arithmetic shift (floor)
//     out[c] = curve[min(max(v[c], 0), 255)]
// Any int16 matrix is legal (3 * 255 * 32768 < 2^31).  Both factors of every product fit 24 bits signed, and the compiler is shown so:
// on the device they are 24-bit multiply-adds with the coefficient a scalar operand, the clamp a median of three.

// coefficient (an int16 value held in an int) times channel (0 .. 255): the sign extension from 16 bits changes nothing and is what
// lets the product be a full-rate 24-bit one
BA_HD int mul24s(int coef, int ch) { return (int)(int16_t)coef * ch; }
// one channel before the curve: the clamped index 0 .. 255
BA_HD uint32_t color_index(const int* m, int r, int g, int b) {
    const int v = (mul24s(m[0], r) + mul24s(m[1], g) + mul24s(m[2], b) + 512) >> 10;
    return (uint32_t)clampi(v, 0, 255);
}
// one pixel, R | G << 8 | B << 16 -> the same
BA_HD uint32_t color_px(uint32_t px, const int* m, const uint8_t* curve) {
#if defined(__HIP_DEVICE_COMPILE__)
    // Opaque to the optimiser, free at run time: the channels are cut out of the packed word here (byte selects of the multiplies)
    // and are visibly 8 bits wide.  Without it the compiler multiplies the demosaic's own red value, whose range it does not see
    // across the phase branches: a quarter-rate v_mul_lo_u32 per channel and tap.
    asm("" : "+v"(px));
#endif
    const int r = (int)(px & 255u), g = (int)((px >> 8) & 255u), b = (int)((px >> 16) & 255u);
    return (uint32_t)curve[color_index(m, r, g, b)] | ((uint32_t)curve[color_index(m + 3, r, g, b)] << 8) |
           ((uint32_t)curve[color_index(m + 6, r, g, b)] << 16);
}

}  // namespace ba
}  // namespace lt
