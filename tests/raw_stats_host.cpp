// Host side of csrc/stats_arith.h (the expressions k_raw_stats.hip runs on the device) for tests/test_raw_stats_cpu.py: built with the
// system C++ compiler, once plain and once with -fsanitize=address,undefined.
//
//   raw_stats_host <case file> <result file>
//
// case file, int32 words: enc, bits, pattern, H, W, pitch, in_r0, in_r1, row0, row1, col0, col1, grid_h, grid_w, lo[4], hi[4], shade,
// black[4] (27 words), then the plane -- pitch * (H - 1) + row bytes, and not one byte more: the byte path must not read past it -- and,
// with shade, the gain plane uint16[H][W].  row1 == 0: the default rows of the run [in_r0, in_r1); col1 == 0: [0, W).
// result file: hist uint32[4][bins], zone_count uint32[grid_h][grid_w], zone_sum uint64[grid_h][grid_w][4], rect int32[4].
// Every pair of sites is read twice -- by byte accesses (pair_at: the surfaces' path) and out of the aligned dwords around it (window_of /
// pair_from_window: the staging frames' path, from a padded copy at each of the four alignments) -- and the two must agree.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stats_arith.h"

using namespace lt;

static int fail(const char* what) {
    std::fprintf(stderr, "raw_stats_host: %s\n", what);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage: raw_stats_host <case file> <result file>");
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return fail("cannot open the case file");
    int32_t hd[27];
    if (std::fread(hd, sizeof(int32_t), 27, f) != 27) return fail("short header");
    const int enc = hd[0], bits = hd[1], pattern = hd[2], H = hd[3], W = hd[4], pitch = hd[5], in_r0 = hd[6], in_r1 = hd[7];
    int row0 = hd[8], row1 = hd[9], col0 = hd[10], col1 = hd[11];
    const int grid_h = hd[12], grid_w = hd[13], shade = hd[22];
    const int32_t *lo = hd + 14, *hi = hd + 18, *black = hd + 23;
    const int rb = st::row_bytes(enc, W);
    const size_t plane_bytes = (size_t)pitch * (size_t)(H - 1) + (size_t)rb;
    uint8_t* plane = static_cast<uint8_t*>(std::malloc(plane_bytes));          // (exactly: ASan sees a read past the last byte)
    if (!plane || std::fread(plane, 1, plane_bytes, f) != plane_bytes) return fail("short plane");
    std::vector<uint16_t> gains;
    if (shade) {
        gains.resize((size_t)H * W);
        if (std::fread(gains.data(), sizeof(uint16_t), gains.size(), f) != gains.size()) return fail("short gain plane");
    }
    std::fclose(f);
    if (row1 == 0) st::default_rows(in_r0, in_r1, &row0, &row1);
    if (col1 == 0) col0 = 0, col1 = W;
    const int ncy = (row1 - row0) / 2, ncx = (col1 - col0) / 2, bins = 1 << bits, smax = bins - 1;
    if (ncy < 1 || ncx < 1 || grid_h < 1 || grid_h > ncy || grid_w < 1 || grid_w > ncx || grid_h > st::GRID_MAX || grid_w > st::GRID_MAX) return fail("bad case");

    // the staging frames' view: the plane inside whole dwords, at each alignment in turn (three bytes of padding either side at most)
    std::vector<std::vector<uint32_t>> padded(4);
    for (int al = 0; al < 4; ++al) {
        padded[(size_t)al].assign((plane_bytes + (size_t)al + 3) / 4 + 1, 0xa5a5a5a5u);
        std::memcpy(reinterpret_cast<uint8_t*>(padded[(size_t)al].data()) + al, plane, plane_bytes);
    }
    const uint32_t mask = (uint32_t)smax;
    auto pair = [&](int y, int x, uint32_t& s0, uint32_t& s1) {
        st::pair_at(enc, plane + (size_t)y * (size_t)pitch, x, mask, s0, s1);
        for (int al = 0; al < 4; ++al) {
            const size_t at = (size_t)al + (size_t)y * (size_t)pitch + (size_t)st::pair_first(enc, x);
            const uint32_t* w = padded[(size_t)al].data() + at / 4;
            const uint32_t w0 = w[0], w1 = st::window_spills((int)(at & 3), st::pair_bytes(enc, x)) ? w[1] : 0u;
            uint32_t t0 = 0, t1 = 0;
            st::pair_from_window(enc, st::window_of(w0, w1, (int)(at & 3)), x, mask, t0, t1);
            if (t0 != s0 || t1 != s1) {
                std::fprintf(stderr, "raw_stats_host: site (%d, %d), alignment %d: window %u %u, bytes %u %u\n", y, x, al, t0, t1, s0, s1);
                std::exit(2);
            }
        }
        if (shade) {
            const uint16_t* g = gains.data() + (size_t)y * W + x;
            const int p0 = ba::phase(pattern, y, x), p1 = ba::phase(pattern, y, x + 1);
            const uint32_t u0 = s0, u1 = s1;
            s0 = st::shaded(u0, black[p0], g[0], smax);
            s1 = st::shaded(u1, black[p1], g[1], smax);
            if (s0 != sa::shade_plain(u0, black[p0], g[0], smax) || s1 != sa::shade_plain(u1, black[p1], g[1], smax)) {       // (the definition's form)
                std::fprintf(stderr, "raw_stats_host: site (%d, %d): shaded differs from shade_plain\n", y, x);
                std::exit(3);
            }
        }
    };
    const st::Bounds b = st::bounds_by_position(pattern, lo, hi);
    std::vector<uint32_t> hist((size_t)4 * bins, 0), count((size_t)grid_h * grid_w, 0);
    std::vector<uint64_t> sum((size_t)grid_h * grid_w * 4, 0);
    for (int cy = 0; cy < ncy; ++cy)
        for (int cx = 0; cx < ncx; ++cx) {
            const int y = row0 + 2 * cy, x = col0 + 2 * cx;
            uint32_t s[4];
            pair(y, x, s[0], s[1]);
            pair(y + 1, x, s[2], s[3]);
            for (int k = 0; k < 4; ++k) {
                if (st::phase_at(pattern, k) != ba::phase(pattern, y + (k >> 1), x + (k & 1))) return fail("phase_at disagrees with ba::phase");
                ++hist[(size_t)st::phase_at(pattern, k) * bins + s[k]];
            }
            if (!st::cell_valid(s[0], s[1], s[2], s[3], b)) continue;
            const size_t zone = (size_t)st::zone_of(cy, grid_h, ncy) * grid_w + (size_t)st::zone_of(cx, grid_w, ncx);
            ++count[zone];
            for (int k = 0; k < 4; ++k) sum[zone * 4 + (size_t)st::phase_at(pattern, k)] += s[k];
        }
    std::free(plane);
    const int32_t rect[4] = {row0, row1, col0, col1};
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return fail("cannot open the result file");
    std::fwrite(hist.data(), sizeof(uint32_t), hist.size(), o);
    std::fwrite(count.data(), sizeof(uint32_t), count.size(), o);
    std::fwrite(sum.data(), sizeof(uint64_t), sum.size(), o);
    std::fwrite(rect, sizeof(int32_t), 4, o);
    std::fclose(o);
    return 0;
}
