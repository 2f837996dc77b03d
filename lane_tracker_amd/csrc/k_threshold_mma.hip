// bilateral_adaptive_threshold (lane_tracker.py:14-83) with the window sums as i8 matrix products, gfx950.
//
//     pass(y, x)  <=>  (left and right)  or  (up and down),      one side:  K p > S + C K,   S = the K pixels on that side
//
// A window sum along a row or a column is a product with a 0/1 band matrix.  Here the band carries the whole side:
//
//     D = K p(y) - sum_{j=1..K} p(y -+ j) - C K - 1  >=  0       <=>  the side passes
//
// so its rows hold +K on the pixel's own position and -1 on the K positions of the side, and sum to zero.  The plane goes in
// as signed bytes p - 128 (one XOR per dword): the offset cancels exactly because of that zero row sum.  Positions outside
// the image enter as pixel value 0 (0x80 after the XOR).  The accumulators start at -C K - 1 (the MFMA's C-in); K <= 35 and
// |p - 128| <= 128 keep everything far inside i32.  A direction passes iff neither side's accumulator is negative: the sign
// bit of (D_a | D_b) is "fails".  No tolerance anywhere: the four partial bit planes are those of k_threshold_walk.hip.
//
// v_mfma_i32_32x32x32_i8 pairs byte j of lane half g of the A operand with byte j of lane half g of the B operand, whatever
// column of the contraction the hardware calls that slot; both operands here are generated with k = 16 g + j, so only that
// pairing is relied on.  The C/D map is the documented one: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//
// Both task kinds compute the TRANSPOSED verdict tile, output row on the lane and 16 output columns in the 16 accumulator
// registers of a lane half, so that a lane collects the bits of its own row without any cross-lane traffic; the two halves
// of a row word meet with one lane exchange per 64 columns.
//
//   * horizontal task: a wave owns 32 rows and walks along x.  The band is the A operand (m = output column, permuted so that
//     lane half g ends up with columns 16 g .. 16 g + 15 of the tile in register order), the plane the B operand (n = row):
//     a lane loads its 16 contiguous bytes of its row straight from global memory, four 32-column blocks (one 128-byte line
//     per row) per trip, two trips ahead.  A sliding window of 4 + 2 NB blocks stays in registers (NB = ceil(K / 32)).
//   * vertical task: a wave owns a strip of 128 columns and walks down the rows in 32-row blocks.  The plane is the A operand
//     (m = dword column c of the strip, k = row): lane (c, g) loads the dword of columns 4c .. 4c+3 of its 16 rows -- every
//     load instruction covers two whole 128-byte lines -- and transposes 4 x 4 bytes with v_perm_b32 into four operands, one
//     per column i of the dword.  The band is the B operand (n = output row).  MFMA set i yields columns 4c + i.
//
// The products use no LDS and no barrier; a horizontal task collects its words in LDS for one contiguous store at its end.  A
// tile whose own pixels are all <= C is written as "fails" without its products ("Dead tiles" below).  Window sizes 15, 20, 35
// as in the walks; the greenery mask (window 65 with the range term) and everything bilateral_walk_supported refuses stay on
// k_threshold_walk.hip / k_threshold.hip.
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "lt_internal.h"

namespace lt {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

template <class F, int... I>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}

__device__ __forceinline__ int xcd_contiguous(int id, int n) {   // see k_threshold.hip
    const int q = n >> 3, r = n & 7, xcd = id & 7, k = id >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

struct MmaArgs {
    const uint8_t* src;                  // u8 plane of frame 0
    unsigned long long *out_h, *out_v;   // partial bit planes of frame 0
    int h, w, wpr;
    int pitch;                           // bytes per row of the plane (a multiple of 64 >= w)
    int C;
    int lds_rows;                        // rows of wpr words a workgroup has in LDS: 32, or 0 when the rows are too wide
    uint32_t live_k, live_all;           // the dead-tile test: 127 - C in every byte; 1 = every block counts as live (see `above`)
    int hgroups;                         // 32-row groups per frame (one horizontal task each)
    int vgroups, vsegs, vseg_len;        // 128-column strips, segments per strip and their length (a multiple of 32)
    int per_frame;                       // tasks per frame
    size_t plane_stride, bits_stride;
};

// The band operands, per lane, built at compile time.  v[form][side][e][lane] = the lane's 16 bytes of the 32 x 32 piece of the
// band that pairs the output tile with input block  d = e - NB (side 0: left / up)  or  d = e (side 1: right / down).
// form 0: the band as A operand, lane m holds output column o(m) with o = reg + 16 g for m = (reg & 3) + 8 (reg >> 2) + 4 g;
// form 1: the band as B operand, lane n holds output row n.  Byte j of lane half g is input position 32 d + 16 g + j.
template <int K>
struct BandTable {
    static constexpr int NB = (K + 31) / 32;
    static constexpr int NOP = NB + 1;
    uint32_t v[2][2][NOP][64][4];
};
constexpr int band_value(int K, int side, int o, int i) {
    if (i == o) return K;
    if (side == 0) return (i >= o - K && i <= o - 1) ? -1 : 0;
    return (i >= o + 1 && i <= o + K) ? -1 : 0;
}
template <int K>
constexpr BandTable<K> make_band() {
    BandTable<K> t{};
    constexpr int NB = BandTable<K>::NB;
    for (int form = 0; form < 2; ++form)
        for (int side = 0; side < 2; ++side)
            for (int e = 0; e <= NB; ++e)
                for (int lane = 0; lane < 64; ++lane) {
                    const int m = lane & 31, g = lane >> 5, d = side == 0 ? e - NB : e;
                    const int o = form == 0 ? (m & 3) + 4 * ((m >> 3) & 3) + 16 * ((m >> 2) & 1) : m;
                    for (int q = 0; q < 4; ++q) {
                        uint32_t word = 0;
                        for (int b = 0; b < 4; ++b)
                            word |= (uint32_t)(band_value(K, side, o, 32 * d + 16 * g + 4 * q + b) & 0xff) << (8 * b);
                        t.v[form][side][e][lane][q] = word;
                    }
                }
    return t;
}
__device__ const BandTable<15> g_band15 = make_band<15>();
__device__ const BandTable<20> g_band20 = make_band<20>();
__device__ const BandTable<35> g_band35 = make_band<35>();
template <int K>
__device__ __forceinline__ const BandTable<K>& band_table() {
    if constexpr (K == 15) return g_band15;
    else if constexpr (K == 20) return g_band20;
    else return g_band35;
}
template <int K, int FORM>
__device__ __forceinline__ void load_band(v4i (&bl)[BandTable<K>::NOP], v4i (&br)[BandTable<K>::NOP], int lane) {
    const BandTable<K>& t = band_table<K>();
#pragma unroll
    for (int e = 0; e < BandTable<K>::NOP; ++e) {
        bl[e] = *reinterpret_cast<const v4i*>(&t.v[FORM][0][e][lane][0]);
        br[e] = *reinterpret_cast<const v4i*>(&t.v[FORM][1][e][lane][0]);
    }
}

__device__ __forceinline__ v16i splat16(int c) {
    v16i v;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = c;
    return v;
}
__device__ __forceinline__ v16i mfma(v4i a, v4i b, v16i c) { return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0); }
__device__ __forceinline__ uint32_t other_half(uint32_t v, int lane) {   // the value of lane ^ 32
    return (uint32_t)__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, (int)v);
}

// trips / tiles between a load and its use.  Depths 1 .. 4 (horizontal) and 1 .. 2 (vertical) measured the same to within the
// run-to-run spread (profiles/NOTES_threshold_mma.md); 3 for the vertical tasks spills at window 35.
template <int K>
struct PrefetchDepth {
    static constexpr int H = 2, V = 2;
};

extern __shared__ unsigned long long task_words[];   // a horizontal task's words, 32 rows of wpr (see mma_h_task)
constexpr int MaxStagedWpr = 128;        // 32 KiB of LDS per wave at the most: wider rows are stored trip by trip

constexpr uint32_t SIGN = 0x80808080u;   // p -> p - 128 in every byte; also pixel value 0 after the flip

// Dead tiles.  C >= 0 and S >= 0, so a pixel p <= C fails K p > S + C K on every side, whatever its neighbours hold: a verdict
// tile whose own pixels are all <= C is all "fails" and needs none of its MFMAs.  `above` collects, in bit 7 of every byte, "this
// byte of x is > C" for C <= 127 (k = 127 - C in every byte: the low seven bits carry into bit 7 from C + 1 on, or bit 7 is set
// already); `any_above` is the wave-uniform answer for the wave's block.  A larger C, or LT_THRESHOLD_SKIP=0 in the experiments
// build, sets MmaArgs::live_all and every block counts as live.  The test runs on the raw bytes with the positions outside the
// image already 0, so those are never live.
__device__ __forceinline__ uint32_t above(uint32_t acc, uint32_t x, uint32_t k) { return acc | ((x & 0x7f7f7f7fu) + k) | x; }
__device__ __forceinline__ uint32_t any_above(uint32_t acc) { return __builtin_amdgcn_ballot_w64((acc & SIGN) != 0u) != 0ull ? 1u : 0u; }

// ---------------------------------------------------------------------------------------------------------------
// Horizontal task: rows 32 grp .. + 31 of a frame, all of its columns.
template <int K>
__device__ __forceinline__ void mma_h_task(const MmaArgs& a, int frame, int grp) {
    constexpr int NB = BandTable<K>::NB, NOP = NB + 1, W = 4 + 2 * NB, D = PrefetchDepth<K>::H;
    const int lane = threadIdx.x, g = lane >> 5;
    const int h = a.h, w = a.w;
    const int row = grp * 32 + (lane & 31);
    const uint8_t* src = a.src + (size_t)frame * a.plane_stride;
    const uint32_t lane_off = (uint32_t)__mul24(min(row, h - 1), a.pitch) + 16u * g;   // the wave-uniform part of an address stays scalar
    unsigned long long* orow = a.out_h + (size_t)frame * a.bits_stride + (size_t)min(row, h - 1) * a.wpr;
    v4i bl[NOP], br[NOP];
    load_band<K, 0>(bl, br, lane);
    const v16i cinit = splat16(-a.C * K - 1);

    // block b = columns 32 b .. 32 b + 31; this lane's piece of it starts at column 32 b + 16 g
    // (a block that lies outside the row's pitch is all masked: any block inside it stands in for its load)
    const int bmax = (a.pitch >> 5) - 1;
    auto fetch = [&](int b) -> v4i { return *reinterpret_cast<const v4i*>(src + 32 * min(max(b, 0), bmax) + lane_off); };
    auto prep = [&](v4i raw, int b, uint32_t& live) -> v4i {      // live: some pixel of the wave's block is > C (wave-uniform)
        const int col = 32 * b + 16 * g;
        if (32 * b < 0 || 32 * b + 32 > w) {          // wave-uniform: a block that reaches over an image edge
#pragma unroll
            for (int q = 0; q < 4; ++q) raw[q] = (col + 4 * q >= 0 && col + 4 * q < w) ? raw[q] : 0;
        }
        v4i v;
        uint32_t acc = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = above(acc, (uint32_t)raw[q], a.live_k);
            v[q] = raw[q] ^ (int)SIGN;
        }
        live = any_above(acc) | a.live_all;
        return v;
    };

    // The window of trip S: blocks 4 S - NB .. 4 S + 3 + NB.  Each trip shifts it by four blocks and takes the four new ones from
    // loads issued D trips earlier: one trip is a few hundred cycles of matrix work, a load from memory takes several times that.
    // Bit i of lv says that win[i] is live; it moves with the window.
    v4i win[W], pf[D][4];
    uint32_t lv = 0u;
#pragma unroll
    for (int i = 4; i < W; ++i) {
        uint32_t live;
        win[i] = prep(fetch(i - 4 - NB), i - 4 - NB, live);
        lv |= live << i;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) win[i] = win[4];      // (shifted out before the first use)
#pragma unroll
    for (int ph = 0; ph < D; ++ph)
#pragma unroll
        for (int i = 0; i < 4; ++i) pf[ph][i] = fetch(4 * ph + NB + i);
    // The task's words, 32 rows of wpr, are one contiguous piece of the bit plane.  A trip yields 16 bytes of each row: stored as
    // they come, every store instruction touches 32 lines and every line is visited by nine trips microseconds apart.  They are
    // collected in LDS in the plane's own layout instead and written out in one contiguous sweep at the end of the task
    // (a.lds_rows = 0: the row is too wide for that, and the words are stored trip by trip).
    const bool staged = a.lds_rows != 0;              // wave-uniform
    unsigned long long* stage = task_words + (lane & 31) * a.wpr;
    const int trips = (w + 127) >> 7;
    for (int sb = 0; sb < trips; sb += D) {
        static_for([&](auto phc) {
            constexpr int ph = decltype(phc)::value;
            const int S = sb + ph;
            if (S < trips) {                          // wave-uniform
#pragma unroll
                for (int i = 0; i < 2 * NB; ++i) win[i] = win[i + 4];
                lv >>= 4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    uint32_t live;
                    win[2 * NB + i] = prep(pf[ph][i], 4 * S + NB + i, live);
                    lv |= live << (2 * NB + i);
                    pf[ph][i] = fetch(4 * (S + D) + NB + i);      // (addresses clamped: any trip may ask)
                }
                // tiles (0, 1) and (2, 3) of the trip: first tile in the high half; a set bit is "fails"
                uint32_t bits[2] = {0xffffffffu, 0xffffffffu};
                if ((lv >> NB) & 15u) {               // wave-uniform: tile u's own block is win[u + NB]
                    static_for([&](auto uc) {
                        constexpr int u = decltype(uc)::value;
                        if ((lv >> (u + NB)) & 1u) {  // wave-uniform
                            v16i accl = cinit, accr = cinit;
                            static_for([&](auto ec) {
                                constexpr int e = decltype(ec)::value;
                                accl = mfma(bl[e], win[u + e], accl);
                                accr = mfma(br[e], win[u + e + NB], accr);
                            }, std::make_integer_sequence<int, NOP>{});
                            // register i of lane half g = column 32 T + 16 g + i: shifted in from the top one, so that bit i is column i
#pragma unroll
                            for (int i = 15; i >= 0; --i)
                                bits[u >> 1] = __builtin_amdgcn_alignbit(bits[u >> 1], (uint32_t)(accl[i] | accr[i]), 31);
                        } else {
                            bits[u >> 1] = (bits[u >> 1] << 16) | 0xffffu;      // a dead tile: sixteen "fails"
                        }
                    }, std::make_integer_sequence<int, 4>{});
                }
                // lane half g writes word 2 S + g of its row: it keeps its own pair of tiles and gets the other half's
                const uint32_t recv = other_half(g ? bits[0] : bits[1], lane);
                const uint32_t p0 = g ? recv : bits[0], p1 = g ? bits[1] : recv;      // columns 0-15 | 16-31 of the two tiles
                const uint32_t lo = __builtin_amdgcn_perm(p1, p0, 0x07060302u), hi = __builtin_amdgcn_perm(p1, p0, 0x05040100u);
                const int word = 2 * S + g;
                const unsigned long long verdict = ~((unsigned long long)lo | ((unsigned long long)hi << 32));
                if (word < a.wpr) {
                    if (staged) stage[word] = verdict;
                    else if (row < h) orow[word] = verdict;
                }
            }
        }, std::make_integer_sequence<int, D>{});
    }
    if (staged) {
        __syncthreads();                              // (the workgroup is this wave)
        const int nwords = min(32, h - grp * 32) * a.wpr;
        unsigned long long* dst = a.out_h + (size_t)frame * a.bits_stride + (size_t)(grp * 32) * a.wpr;
        for (int i = lane; i < nwords; i += 64) dst[i] = task_words[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Vertical task: columns 128 grp .. + 127, rows [y0, y1) (y0 a multiple of 32).
template <int K>
__device__ __forceinline__ void mma_v_task(const MmaArgs& a, int frame, int grp, int seg) {
    constexpr int NB = BandTable<K>::NB, NOP = NB + 1, W = 2 * NB + 1, D = PrefetchDepth<K>::V;
    const int lane = threadIdx.x, g = lane >> 5;
    const int h = a.h, w = a.w;
    const int y0 = seg * a.vseg_len, y1 = min(y0 + a.vseg_len, h);
    if (y0 >= h) return;
    const int col = grp * 128 + 4 * (lane & 31);
    const bool colok = col < w;
    const uint8_t* src = a.src + (size_t)frame * a.plane_stride;
    const uint32_t colc = (uint32_t)min(col, w - 4);
    const uint32_t lane_off = (uint32_t)__mul24(16 * g, a.pitch) + colc;   // blocks inside the image: the row part of an address stays scalar
    unsigned long long* out = a.out_v + (size_t)frame * a.bits_stride;
    v4i bl[NOP], br[NOP];
    load_band<K, 1>(bl, br, lane);
    const v16i cinit = splat16(-a.C * K - 1);

    struct Raw { uint32_t r[16]; };
    struct Block { v4i op[4]; };                      // op[i]: column 4 c + i, rows 32 b + 16 g + 0 .. 15 in byte order
    auto fetch = [&](int b) -> Raw {
        Raw x;
        if (b >= 0 && 32 * b + 32 <= h) {             // wave-uniform
            const uint8_t* base = src + (size_t)(32 * b) * a.pitch;
#pragma unroll
            for (int j = 0; j < 16; ++j) x.r[j] = *reinterpret_cast<const uint32_t*>(base + (size_t)j * a.pitch + lane_off);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int r = 32 * b + 16 * g + j;
                x.r[j] = *reinterpret_cast<const uint32_t*>(src + (uint32_t)__mul24(min(max(r, 0), h - 1), a.pitch) + colc);
            }
        }
        return x;
    };
    auto prep = [&](const Raw& x, int b, uint32_t& live) -> Block {      // live: some pixel of the wave's block is > C (wave-uniform)
        Block o;
        const bool inside = 32 * b >= 0 && 32 * b + 32 <= h && grp * 128 + 128 <= w;      // wave-uniform
        uint32_t acc = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t r[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int y = 32 * b + 16 * g + 4 * q + t;
                uint32_t raw = x.r[4 * q + t];
                if (!inside) raw = (colok && y >= 0 && y < h) ? raw : 0u;
                acc = above(acc, raw, a.live_k);
                r[t] = raw ^ SIGN;
            }
            // 4 x 4 byte transpose: rows r[0..3] with columns in their bytes -> columns with rows in their bytes
            const uint32_t a01 = __builtin_amdgcn_perm(r[1], r[0], 0x05010400u), b01 = __builtin_amdgcn_perm(r[1], r[0], 0x07030602u);
            const uint32_t a23 = __builtin_amdgcn_perm(r[3], r[2], 0x05010400u), b23 = __builtin_amdgcn_perm(r[3], r[2], 0x07030602u);
            o.op[0][q] = (int)__builtin_amdgcn_perm(a23, a01, 0x05040100u);
            o.op[1][q] = (int)__builtin_amdgcn_perm(a23, a01, 0x07060302u);
            o.op[2][q] = (int)__builtin_amdgcn_perm(b23, b01, 0x05040100u);
            o.op[3][q] = (int)__builtin_amdgcn_perm(b23, b01, 0x07060302u);
        }
        live = any_above(acc) | a.live_all;
        return o;
    };

    // The window of tile T: blocks T - NB .. T + NB.  Each tile shifts it by one block and takes the new one from loads issued D
    // tiles earlier (see the horizontal task).  Bit i of lv says that win[i] is live; it moves with the window.
    const int t_first = y0 >> 5, t_end = (y1 + 31) >> 5;
    Block win[W];
    Raw pf[D];
    uint32_t lv = 0u;
#pragma unroll
    for (int i = 1; i < W; ++i) {
        uint32_t live;
        win[i] = prep(fetch(t_first - NB + i - 1), t_first - NB + i - 1, live);
        lv |= live << i;
    }
    win[0] = win[1];                                  // (shifted out before the first use)
#pragma unroll
    for (int ph = 0; ph < D; ++ph) pf[ph] = fetch(t_first + NB + ph);
    for (int tb = t_first; tb < t_end; tb += D) {
        static_for([&](auto phc) {
            constexpr int ph = decltype(phc)::value;
            const int T = tb + ph;
            if (T < t_end) {                          // wave-uniform
#pragma unroll
                for (int i = 0; i + 1 < W; ++i) win[i] = win[i + 1];
                uint32_t live;
                win[W - 1] = prep(pf[ph], T + NB, live);
                lv = (lv >> 1) | (live << (W - 1));
                pf[ph] = fetch(T + NB + D);
                unsigned long long verdict = 0ull;    // a dead tile (its own block is win[NB]): nothing passes
                if ((lv >> NB) & 1u) {                // wave-uniform
                    uint32_t x = 0u, y = 0u;          // fail bits of columns 32 t + 16 g + 0..15: t = 0 | 1 << 16 in x, t = 2 | 3 << 16 in y
                    static_for([&](auto ic) {
                        constexpr int i = decltype(ic)::value;
                        v16i accl = cinit, accr = cinit;
                        static_for([&](auto ec) {
                            constexpr int e = decltype(ec)::value;
                            accl = mfma(win[e].op[i], bl[e], accl);
                            accr = mfma(win[e + NB].op[i], br[e], accr);
                        }, std::make_integer_sequence<int, NOP>{});
                        // register j of lane half g = dword column (j & 3) + 8 (j >> 2) + 4 g, i.e. column 32 (j >> 2) + 16 g + 4 (j & 3) + i
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            const uint32_t s = (uint32_t)(accl[j] | accr[j]) >> 31;
                            const int pos = 16 * ((j >> 2) & 1) + 4 * (j & 3) + i;
                            if (j < 8) x |= s << pos;
                            else y |= s << pos;
                        }
                    }, std::make_integer_sequence<int, 4>{});
                    // lane half g writes word 2 grp + g of the row
                    const uint32_t recv = other_half(g ? x : y, lane);
                    const uint32_t p0 = g ? recv : x, p1 = g ? y : recv;
                    const uint32_t lo = __builtin_amdgcn_perm(p1, p0, 0x05040100u), hi = __builtin_amdgcn_perm(p1, p0, 0x07060302u);
                    verdict = ~((unsigned long long)lo | ((unsigned long long)hi << 32));
                }
                const int row = 32 * T + (lane & 31), word = 2 * grp + g;
                if (row < y1 && word < a.wpr) out[(size_t)row * a.wpr + word] = verdict;
            }
        }, std::make_integer_sequence<int, D>{});
    }
}

// Both passes of a plane in one launch.  Workgroup b runs on XCD b % 8: the launch order is renumbered so that every XCD owns a
// contiguous range of tasks, and tasks are numbered frame by frame with the horizontal and vertical tasks of a frame alternating,
// so a frame's plane is read by one XCD in one stretch of time (as in k_bilateral_walk_hv).
template <int K>
__global__ __launch_bounds__(64, 2) void k_bilateral_mma_hv(MmaArgs a) {
    const int b = xcd_contiguous(blockIdx.x, gridDim.x);
    const int frame = b / a.per_frame, j = b - frame * a.per_frame;
    const int nh = a.hgroups, nv = a.vgroups * a.vsegs, pairs = min(nh, nv);
    int v;                                            // vertical task number, or -1 - horizontal task number
    if (j < 2 * pairs) v = (j & 1) ? (j >> 1) : -1 - (j >> 1);
    else v = nh > pairs ? -1 - (j - pairs) : j - pairs;
    if (v < 0) mma_h_task<K>(a, frame, -1 - v);
    else mma_v_task<K>(a, frame, v / a.vsegs, v % a.vsegs);
}

template <int K>
void launch_mma(hipStream_t s, const uint8_t* src, int C, unsigned long long* out_h, unsigned long long* out_v, int h, int w, int pitch,
                size_t plane_stride, size_t bits_stride, int n, bool skip, bool stage) {
    MmaArgs a;
    a.src = src;
    a.out_h = out_h; a.out_v = out_v;
    a.h = h; a.w = w; a.wpr = (w + 63) / 64;
    a.pitch = pitch;
    a.C = C;
    a.live_all = (skip && C <= 127) ? 0u : 1u;          // the byte test of `above` holds for C <= 127: beyond it nothing is skipped
    a.live_k = a.live_all ? 0u : (uint32_t)(127 - C) * 0x01010101u;
    a.hgroups = (h + 31) / 32;
    a.vgroups = (w + 127) / 128;
    a.vsegs = h > 640 ? 2 : 1;                        // the walks' split of the rows, on 32-row tile boundaries
    a.vseg_len = a.vsegs == 1 ? ((h + 31) & ~31) : (((h + 1) / 2 + 31) & ~31);
    a.per_frame = a.hgroups + a.vgroups * a.vsegs;
    a.plane_stride = plane_stride;
    a.bits_stride = bits_stride;
    a.lds_rows = (stage && a.wpr <= MaxStagedWpr) ? 32 : 0;
    hipLaunchKernelGGL((k_bilateral_mma_hv<K>), dim3((unsigned)(a.per_frame * n)), dim3(64), (size_t)a.lds_rows * a.wpr * sizeof(unsigned long long), s, a);
}

void dispatch_mma(int k, hipStream_t s, const uint8_t* src, int C, unsigned long long* out_h, unsigned long long* out_v, int h, int w,
                  int pitch, size_t plane_stride, size_t bits_stride, int n, bool skip, bool stage) {
    switch (k) {
        case 15: launch_mma<15>(s, src, C, out_h, out_v, h, w, pitch, plane_stride, bits_stride, n, skip, stage); break;
        case 20: launch_mma<20>(s, src, C, out_h, out_v, h, w, pitch, plane_stride, bits_stride, n, skip, stage); break;
        default: launch_mma<35>(s, src, C, out_h, out_v, h, w, pitch, plane_stride, bits_stride, n, skip, stage); break;
    }
}

}  // namespace

// Both bilateral thresholds as band products: the four partial bit planes of launch_bilateral_walk, bit for bit.  0 = ran,
// -1 = bilateral_walk_supported says no, 1 = switched off (experiments build, LT_THRESHOLD_MMA=0: the caller takes the walks).
int launch_bilateral_mma(hipStream_t s, const uint8_t* thr, int k_r, int C_r, const uint8_t* thb, int k_b, int C_b,
                         unsigned long long* merged, unsigned long long* s1, unsigned long long* s2, unsigned long long* s3,
                         int h, int w, int pitch, size_t plane_stride, size_t bits_stride, int n) {
    if (n <= 0 || !bilateral_walk_supported(k_r, C_r, k_b, C_b, h, w, pitch, plane_stride)) return -1;
    static const bool off = [] { const char* e = LT_EXP_ENV("LT_THRESHOLD_MMA"); return e && e[0] == '0'; }();
    if (off) return 1;
    static const bool skip = [] { const char* e = LT_EXP_ENV("LT_THRESHOLD_SKIP"); return !(e && e[0] == '0'); }();   // A/B: 0 = every block live
    static const bool stage = [] { const char* e = LT_EXP_ENV("LT_THRESHOLD_STAGE"); return !(e && e[0] == '0'); }();   // A/B: 0 = words stored trip by trip
    dispatch_mma(k_r, s, thr, C_r, merged, s1, h, w, pitch, plane_stride, bits_stride, n, skip, stage);
    dispatch_mma(k_b, s, thb, C_b, s2, s3, h, w, pitch, plane_stride, bits_stride, n, skip, stage);
    return 0;
}

namespace { __global__ void k_preload_k_threshold_mma() {} }
void preload_k_threshold_mma(hipStream_t s) { hipLaunchKernelGGL(k_preload_k_threshold_mma, dim3(1), dim3(1), 0, s); }

}  // namespace lt
