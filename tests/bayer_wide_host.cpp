// The wide raw table's expression of csrc/bayer_arith.h (lut_row_wide, condition4w, condition1w) on the host, as the 10- / 12-bit walk and
// row conversion of k_frontend.hip run it: a 4 x 4 window of 16-bit sites at site (by, bx), every row two dwords, its rows 0, 2 conditioned
// with the table rows of (by & 1, bx & 1) / (by & 1, ~bx & 1), its rows 1, 3 with those of the other row parity.
//
//   bayer_wide_host PATTERN BITS LUT.bin WINDOWS.bin OUT.bin
//
// LUT.bin: 4 << BITS bytes, phase-major.  WINDOWS.bin: n windows of 16 little-endian 16-bit words, row-major.  OUT.bin: per window and per
// parity pair (by & 1, bx & 1) = (0,0), (0,1), (1,0), (1,1) the four conditioned window rows as little-endian dwords of four bytes, then the
// same 16 sites once more through condition1w.  The table lives in a heap block of exactly 4 << BITS bytes (the sanitizer build: any lookup
// outside it -- a mask that lets a high bit through -- is an error).  Prints "ok <n>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bayer_arith.h"

namespace ba = lt::ba;

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const int pattern = std::atoi(argv[1]), bits = std::atoi(argv[2]);
    if (pattern < 0 || pattern > 3 || (bits != 10 && bits != 12)) return 2;
    const size_t lut_bytes = (size_t)4 << bits;
    const std::vector<uint8_t> table = slurp(argv[3]), win = slurp(argv[4]);
    if (table.size() != lut_bytes || win.empty() || win.size() % 32) return 2;
    uint8_t* lut = static_cast<uint8_t*>(std::malloc(lut_bytes));
    if (!lut) return 3;
    std::memcpy(lut, table.data(), lut_bytes);
    const uint32_t mask = (1u << bits) - 1u;
    const size_t n = win.size() / 32;
    std::vector<uint32_t> out;
    out.reserve(n * 4 * 8);
    for (size_t i = 0; i < n; ++i) {
        uint32_t lo[4], hi[4];
        for (int k = 0; k < 4; ++k) {                         // (little-endian host: word c of a row is column c)
            std::memcpy(&lo[k], &win[32 * i + 8 * k], 4);
            std::memcpy(&hi[k], &win[32 * i + 8 * k + 4], 4);
        }
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                const uint8_t *ea = lut + ba::lut_row_wide(bits, pattern, py, px), *eb = lut + ba::lut_row_wide(bits, pattern, py, px ^ 1);
                const uint8_t *oa = lut + ba::lut_row_wide(bits, pattern, py ^ 1, px), *ob = lut + ba::lut_row_wide(bits, pattern, py ^ 1, px ^ 1);
                out.push_back(ba::condition4w(lo[0], hi[0], ea, eb, mask));
                out.push_back(ba::condition4w(lo[1], hi[1], oa, ob, mask));
                out.push_back(ba::condition4w(lo[2], hi[2], ea, eb, mask));
                out.push_back(ba::condition4w(lo[3], hi[3], oa, ob, mask));
                for (int k = 0; k < 4; ++k) {                 // the same, a site at a time (the byte-wise row conversion)
                    uint32_t w = 0;
                    for (int c = 0; c < 4; ++c) {
                        const uint32_t s = ((c < 2 ? lo[k] : hi[k]) >> (16 * (c & 1))) & 0xffffu;
                        w |= ba::condition1w(s, lut + ba::lut_row_wide(bits, pattern, py ^ (k & 1), px ^ (c & 1)), mask) << (8 * c);
                    }
                    out.push_back(w);
                }
            }
    }
    std::free(lut);
    FILE* f = std::fopen(argv[5], "wb");
    if (!f) return 3;
    const size_t wrote = std::fwrite(out.data(), 4, out.size(), f);
    std::fclose(f);
    if (wrote != out.size()) return 3;
    std::printf("ok %zu\n", n);
    return 0;
}
