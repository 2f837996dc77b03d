// Raw Bayer statistics (lt_raw_stats) -- per-colour histograms and the zone sums of an auto-white-balance step -- as plain inline
// functions without HIP types: k_raw_stats.hip runs exactly these expressions on the device, and a host program (tests/raw_stats_host.cpp)
// compiles the same header with the system compiler, so the CPU tests check what the GPU runs.
//
// Statistics are taken of the samples as they enter the raw table: the byte, the 16-bit word masked to its bits, the unpacked sample of a
// MIPI-packed row (mipi_arith.h), each taken through the shading map first where there is one (shade_arith.h).  The rectangle -- rows
// [row0, row1), columns [col0, col1), all even -- is tiled by 2 x 2 cells anchored at even coordinates, so a cell holds one site of each
// colour phase (bayer_arith.h: phase): ncy x ncx cells.
//   hist[p][v]            sites of phase p in the rectangle whose sample is v; every site counts
//   zone of cell (cy, cx) (cy * grid_h / ncy, cx * grid_w / ncx), integer division; 1 <= grid_h <= min(64, ncy), likewise grid_w
//   a cell is valid       when all four of its samples s_p satisfy lo[p] <= s_p <= hi[p]
//   zone_count, zone_sum  the valid cells of a zone, and the per-phase sums of their samples
// A cell is handled by POSITION -- k = 2 * (row parity) + (column parity) inside the cell, k = 0 its top-left site -- and what is given by
// phase (bounds, pedestals, histogram rows) is brought into that order once per call: phase_at(pattern, k).
#pragma once
#include <cstdint>

#include "bayer_arith.h"
#include "mipi_arith.h"
#include "shade_arith.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ST_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ST_HD inline
#endif

namespace lt {
namespace st {

constexpr int GRID_MAX = 64;
// how a row holds its samples
constexpr int ENC_BYTES = 0, ENC_WORDS = 1, ENC_RAW10 = 2, ENC_RAW12 = 3;
ST_HD constexpr int pack_of(int enc) { return enc == ENC_RAW10 ? ma::PACK10 : enc == ENC_RAW12 ? ma::PACK12 : -1; }
// the bytes of a row of w sites
ST_HD constexpr int row_bytes(int enc, int w) { return enc == ENC_BYTES ? w : enc == ENC_WORDS ? 2 * w : ma::row_bytes(pack_of(enc), w); }

// The default rows: the run [r0, r1) that lt_get_input_rows names -- the rows every upload entry point brings --, rounded inward to even.
ST_HD void default_rows(int r0, int r1, int* row0, int* row1) {
    *row0 = (r0 + 1) & ~1;
    *row1 = r1 & ~1;
}
// the phase of the site at position k of a cell (cells are anchored at even coordinates)
ST_HD constexpr int phase_at(int pattern, int k) { return ba::phase(pattern, k >> 1, k & 1); }
// the zone of cell c along an axis of ncells cells under a grid of `grid` zones (c < 8192, grid <= 64: below 2^19)
ST_HD int zone_of(int c, int grid, int ncells) { return (int)((uint32_t)c * (uint32_t)grid / (uint32_t)ncells); }
// The bounds of a cell's four sites, by position.
struct Bounds { int32_t lo[4], hi[4]; };
ST_HD Bounds bounds_by_position(int pattern, const int32_t* lo, const int32_t* hi) {
    Bounds b{};
    for (int k = 0; k < 4; ++k) { b.lo[k] = lo[phase_at(pattern, k)]; b.hi[k] = hi[phase_at(pattern, k)]; }
    return b;
}
ST_HD bool in_bounds(uint32_t s, int lo, int hi) { return (int)s >= lo && (int)s <= hi; }
ST_HD bool cell_valid(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, const Bounds& b) {
    return in_bounds(s0, b.lo[0], b.hi[0]) && in_bounds(s1, b.lo[1], b.hi[1]) && in_bounds(s2, b.lo[2], b.hi[2]) && in_bounds(s3, b.lo[3], b.hi[3]);
}

// ---- the two sites x, x + 1 (x even) of a row: one row of a cell ----------------------------------------------------------------------
// Byte accesses, no byte outside the pair's own: what reads a caller's surface at any alignment.  mask = (1 << bits) - 1.
ST_HD void pair_at(int enc, const uint8_t* row, int x, uint32_t mask, uint32_t& s0, uint32_t& s1) {
    if (enc == ENC_BYTES) {
        s0 = row[x], s1 = row[x + 1];
    } else if (enc == ENC_WORDS) {
        s0 = ((uint32_t)row[2 * x] | ((uint32_t)row[2 * x + 1] << 8)) & mask;
        s1 = ((uint32_t)row[2 * x + 2] | ((uint32_t)row[2 * x + 3] << 8)) & mask;
    } else {
        s0 = ma::site_at(pack_of(enc), row, x), s1 = ma::site_at(pack_of(enc), row, x + 1);
    }
}
// The same from a window: the bytes the pair lies in -- pair_bytes(enc, x) of them from byte pair_first(enc, x) of the row, at most five --
// as the low bytes of a 64-bit value, byte 0 the first.  What reads a slot's staging frame in aligned dwords.
ST_HD constexpr int pair_first(int enc, int x) { return enc == ENC_BYTES ? x : enc == ENC_WORDS ? 2 * x : ma::high_byte(pack_of(enc), x); }
ST_HD constexpr int pair_bytes(int enc, int x) { return enc == ENC_BYTES ? 2 : enc == ENC_WORDS ? 4 : enc == ENC_RAW12 ? 3 : (x & 2) ? 3 : 5; }
// one packed site of the window that starts at byte `first` of its row: ma::site_at's expression on the window's bytes
ST_HD uint32_t window_site(int pack, uint64_t v, int first, int x) {
    const uint32_t h = (uint32_t)(v >> (8 * (ma::high_byte(pack, x) - first))) & 255u, l = (uint32_t)(v >> (8 * (ma::low_byte(pack, x) - first))) & 255u;
    return pack == ma::PACK10 ? (h << 2) | ((l >> ma::low_shift(pack, x)) & 3u) : (h << 4) | ((l >> ma::low_shift(pack, x)) & 15u);
}
ST_HD void pair_from_window(int enc, uint64_t v, int x, uint32_t mask, uint32_t& s0, uint32_t& s1) {
    if (enc == ENC_BYTES) {
        s0 = (uint32_t)v & 255u, s1 = (uint32_t)(v >> 8) & 255u;
    } else if (enc == ENC_WORDS) {
        s0 = (uint32_t)v & mask, s1 = (uint32_t)(v >> 16) & mask;
    } else {
        const int first = pair_first(enc, x);
        s0 = window_site(pack_of(enc), v, first, x), s1 = window_site(pack_of(enc), v, first, x + 1);
    }
}
// The window from the aligned dwords around it: w0 holds byte `at` of the row's memory at its byte at & 3, w1 is the next dword (read only
// where window_spills says the window reaches it).
ST_HD constexpr bool window_spills(int at, int nbytes) { return (at & 3) + nbytes > 4; }
ST_HD uint64_t window_of(uint32_t w0, uint32_t w1, int at) { return (((uint64_t)w1 << 32) | w0) >> (8 * (at & 3)); }

// a sample through the shading map: shade_arith.h's expression with the pedestal's rounding term folded in, as the walks run it
ST_HD uint32_t shaded(uint32_t s, int black, uint32_t gain, int smax) { return sa::shade(s, black, sa::round_term(black), gain, smax); }

}  // namespace st
}  // namespace lt
