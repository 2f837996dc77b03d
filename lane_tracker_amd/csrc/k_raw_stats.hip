// Raw Bayer statistics (lt_raw_stats; stats_arith.h holds the definition and every expression): per-colour histograms and the zone sums of
// an auto-white-balance step, of the samples as they enter the raw table.
//   k_raw_stats<ENC, BITS, SURF, SHADE>   grid (bands of BAND cell rows, PARTS, slots), 256 threads
//     ENC, BITS  how a row holds its samples: bytes (8), 16-bit words (10, 12), RAW10 (10), RAW12 (12)
//     SURF       the frames are the caller's surfaces, entry z of the launch's piece of the surface table (any pitch, any alignment): byte
//                accesses, none outside the pair's own bytes.  Else the slots' staging frames: the aligned dwords that hold a pair's bytes
//                (one, or two where the pair crosses a dword), shifted into place -- at most three bytes either side of the pair, inside the
//                slot's staging frame or the padding behind the last one
//     SHADE      every sample through the shading map first: its gain from the plane the context expands (one dword for a pair)
// A thread owns whole 2 x 2 cells -- column cx of the band, cell row after cell row -- so validity is local and its zone column is fixed:
// it sums the valid cells of a zone in registers and adds them to the workgroup's zone sums in LDS when the zone row changes.  The
// histogram of the workgroup is in LDS (ds_add_u32, no return value); both are merged into the slot's zeroed output with atomicAdd
// (uint32 counts, 64-bit sums), zeros skipped.  Every quantity is an integer count or sum: any order gives the same bits.
//   LDS: BITS 8: 4 KB of histogram, 10: 16 KB, 12: 32 KB -- at 12 bits all four phases would be the whole 64 KB, so the two rows of the
//   cells go to two workgroups (PARTS 2): part 0 counts the top row's two phases and makes the zone sums (it reads both rows), part 1
//   reads and counts the bottom row alone -- plus 21.25 KB of zone sums: a band of 16 cell rows touches at most 17 zone rows (grid_h <=
//   ncy) of at most 64 zones of five words.  53.25 KB at most: two workgroups a CU at 12 bits, four and more below.
//   The zone sums in LDS are uint32: a band holds at most 16 x 8192 cells of samples below 4096, under 2^29.
#include "lt_internal.h"
#include "stats_arith.h"

namespace lt {
namespace {

constexpr int BAND = 16, ZONE_ROWS = BAND + 1, THREADS = 256;

struct StatsArgs {
    const SurfEntry* tab;          // SURF: the table's entry of the launch's first slot
    const uint8_t* frames;         // else: the staging frame of the launch's first slot, `stride` bytes a slot, rows of `pitch` bytes
    size_t stride;
    int pitch;
    const uint16_t* gains;         // SHADE: uint16[img_h][img_w]
    int img_w;
    int row0, col0, ncy, ncx, grid_h, grid_w;
    st::Bounds b;                  // by position in the cell
    int black[4];                  // likewise
    int p0;                        // the phase of the cell's top-left site; position k has phase p0 ^ k
    uint32_t* hist;                // of the launch's first slot: [4][bins]
    uint32_t* zone_count;          // [grid_h][grid_w]
    unsigned long long* zone_sum;  // [grid_h][grid_w][4], by phase
};

// the sites x, x + 1 of the row at `row`; SHADE: corrected with the gains at `g` and the pedestals ka, kb
template <int ENC, int BITS, bool SURF, bool SHADE>
__device__ __forceinline__ void row_pair(const uint8_t* row, int x, const uint16_t* g, int ka, int kb, uint32_t& s0, uint32_t& s1) {
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    if (SURF) {
        st::pair_at(ENC, row, x, MASK, s0, s1);
    } else {
        const uintptr_t at = (uintptr_t)(row + st::pair_first(ENC, x));
        const uint32_t* w = reinterpret_cast<const uint32_t*>(at & ~(uintptr_t)3);
        const uint32_t w0 = w[0], w1 = st::window_spills((int)(at & 3), st::pair_bytes(ENC, x)) ? w[1] : 0u;
        st::pair_from_window(ENC, st::window_of(w0, w1, (int)(at & 3)), x, MASK, s0, s1);
    }
    if (SHADE) {
        const uint32_t gg = *reinterpret_cast<const uint32_t*>(g);        // (x and img_w even: a dword of its own)
        s0 = st::shaded(s0, ka, gg & 0xffffu, (int)MASK);
        s1 = st::shaded(s1, kb, gg >> 16, (int)MASK);
    }
}

template <int ENC, int BITS, bool SURF, bool SHADE>
__global__ __launch_bounds__(THREADS) void k_raw_stats(const StatsArgs a) {
    constexpr int BINS = 1 << BITS, PARTS = BITS == 12 ? 2 : 1, HW = 4 / PARTS * BINS;
    __shared__ uint32_t hist[HW];
    __shared__ uint32_t zone[ZONE_ROWS * st::GRID_MAX * 5];
    const int tid = (int)threadIdx.x, z = (int)blockIdx.z, part = PARTS == 2 ? (int)blockIdx.y : 0;
    const bool top = PARTS == 1 || part == 0, bottom = PARTS == 1 || part == 1, zones = part == 0;
    const int cy0 = (int)blockIdx.x * BAND, cy1 = min(cy0 + BAND, a.ncy);
    const int zy0 = st::zone_of(cy0, a.grid_h, a.ncy), zwords = (st::zone_of(cy1 - 1, a.grid_h, a.ncy) - zy0 + 1) * a.grid_w;
    if (zwords > ZONE_ROWS * st::GRID_MAX) return;                       // (never: grid_h <= ncy, grid_w <= 64 are checked on the host)
    for (int i = tid; i < HW; i += THREADS) hist[i] = 0;
    if (zones)
        for (int i = tid; i < zwords * 5; i += THREADS) zone[i] = 0;
    __syncthreads();

    const uint8_t* base;
    int pitch;
    if (SURF) {
        const SurfEntry e = a.tab[z];
        base = reinterpret_cast<const uint8_t*>(e.plane[0]);
        pitch = e.pitch;
    } else {
        base = a.frames + (size_t)z * a.stride;
        pitch = a.pitch;
    }
    // the histogram row of the site at position k: PARTS 1 its phase; PARTS 2 the column bit of its phase (the row bit is the part's)
    const int h0 = (PARTS == 1 ? a.p0 : a.p0 & 1) * BINS, h1 = (PARTS == 1 ? a.p0 ^ 1 : (a.p0 & 1) ^ 1) * BINS;
    const int h2 = PARTS == 1 ? (a.p0 ^ 2) * BINS : h0, h3 = PARTS == 1 ? (a.p0 ^ 3) * BINS : h1;

    for (int cx = tid; cx < a.ncx; cx += THREADS) {
        const int x = a.col0 + 2 * cx, zx = st::zone_of(cx, a.grid_w, a.ncx);
        uint32_t cnt = 0, q0 = 0, q1 = 0, q2 = 0, q3 = 0;
        int cur = zy0;
        auto flush = [&]() {
            if (cnt) {
                uint32_t* q = &zone[((cur - zy0) * a.grid_w + zx) * 5];
                atomicAdd(q, cnt), atomicAdd(q + 1, q0), atomicAdd(q + 2, q1), atomicAdd(q + 3, q2), atomicAdd(q + 4, q3);
            }
            cnt = q0 = q1 = q2 = q3 = 0;
        };
        for (int cy = cy0; cy < cy1; ++cy) {
            const int y = a.row0 + 2 * cy;
            const uint8_t* row = base + (size_t)y * (size_t)pitch;
            const uint16_t* g = SHADE ? a.gains + (size_t)y * (size_t)a.img_w + x : nullptr;
            uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            if (top || zones) row_pair<ENC, BITS, SURF, SHADE>(row, x, g, a.black[0], a.black[1], s0, s1);
            if (bottom || zones) row_pair<ENC, BITS, SURF, SHADE>(row + pitch, x, SHADE ? g + a.img_w : nullptr, a.black[2], a.black[3], s2, s3);
            if (top) atomicAdd(&hist[h0 + s0], 1u), atomicAdd(&hist[h1 + s1], 1u);
            if (bottom) atomicAdd(&hist[h2 + s2], 1u), atomicAdd(&hist[h3 + s3], 1u);
            if (zones) {
                const int zy = st::zone_of(cy, a.grid_h, a.ncy);
                if (zy != cur) { flush(); cur = zy; }
                if (st::cell_valid(s0, s1, s2, s3, a.b)) { ++cnt; q0 += s0; q1 += s1; q2 += s2; q3 += s3; }
            }
        }
        if (zones) flush();
    }
    __syncthreads();

    uint32_t* gh = a.hist + (size_t)z * 4 * BINS;
    const int row_bit = ((a.p0 >> 1) ^ part) & 1;                      // PARTS 2: the row bit of the phases this part counted
    for (int i = tid; i < HW; i += THREADS) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(&gh[PARTS == 1 ? i : 2 * row_bit * BINS + i], v);
    }
    if (!zones) return;
    const size_t zbase = (size_t)z * a.grid_h * a.grid_w + (size_t)zy0 * a.grid_w;      // LDS zone i is zone zy0 * grid_w + i of the slot
    for (int i = tid; i < zwords; i += THREADS) {
        const uint32_t* q = &zone[i * 5];
        if (!q[0]) continue;                                           // (no valid cell: no sum either)
        atomicAdd(&a.zone_count[zbase + i], q[0]);
        for (int k = 0; k < 4; ++k) atomicAdd(&a.zone_sum[(zbase + i) * 4 + (a.p0 ^ k)], (unsigned long long)q[1 + k]);
    }
}

template <int ENC, int BITS>
void launch_form(hipStream_t s, dim3 grid, const StatsArgs& a, bool surf, bool shade) {
    if (surf && shade) hipLaunchKernelGGL((k_raw_stats<ENC, BITS, true, true>), grid, dim3(THREADS), 0, s, a);
    else if (surf) hipLaunchKernelGGL((k_raw_stats<ENC, BITS, true, false>), grid, dim3(THREADS), 0, s, a);
    else if (shade) hipLaunchKernelGGL((k_raw_stats<ENC, BITS, false, true>), grid, dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL((k_raw_stats<ENC, BITS, false, false>), grid, dim3(THREADS), 0, s, a);
}

}  // namespace

void launch_raw_stats(hipStream_t s, FrameSource src, int first_slot, int n, const RawStatsJob& j) {
    if (n <= 0 || j.ncy <= 0 || j.ncx <= 0) return;
    const int enc = j.pack == 0 ? st::ENC_RAW10 : j.pack == 1 ? st::ENC_RAW12 : j.bits == 8 ? st::ENC_BYTES : st::ENC_WORDS;
    StatsArgs a{};
    a.tab = src.tab ? src.tab + first_slot : nullptr;
    a.frames = src.frames;
    a.stride = src.stride;
    a.pitch = st::row_bytes(enc, j.img_w);
    a.gains = j.gains;
    a.img_w = j.img_w;
    a.row0 = j.row0, a.col0 = j.col0, a.ncy = j.ncy, a.ncx = j.ncx, a.grid_h = j.grid_h, a.grid_w = j.grid_w;
    a.b = st::bounds_by_position(j.pattern, j.lo, j.hi);
    for (int k = 0; k < 4; ++k) a.black[k] = j.blk.b[st::phase_at(j.pattern, k)];
    a.p0 = st::phase_at(j.pattern, 0);
    a.hist = j.hist, a.zone_count = j.zone_count, a.zone_sum = j.zone_sum;
    const dim3 grid((unsigned)((j.ncy + BAND - 1) / BAND), j.bits == 12 ? 2u : 1u, (unsigned)n);
    const bool surf = src.tab != nullptr, shade = j.gains != nullptr;
    if (enc == st::ENC_BYTES) launch_form<st::ENC_BYTES, 8>(s, grid, a, surf, shade);
    else if (enc == st::ENC_RAW10) launch_form<st::ENC_RAW10, 10>(s, grid, a, surf, shade);
    else if (enc == st::ENC_RAW12) launch_form<st::ENC_RAW12, 12>(s, grid, a, surf, shade);
    else if (j.bits == 10) launch_form<st::ENC_WORDS, 10>(s, grid, a, surf, shade);
    else launch_form<st::ENC_WORDS, 12>(s, grid, a, surf, shade);
}

}  // namespace lt
