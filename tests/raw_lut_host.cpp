// The raw table's expression of csrc/bayer_arith.h (lut_row, condition4, condition1) on the host, as the conditioned walk and row
// conversion of k_frontend.hip run it: a 4 x 4 window of bytes at site (by, bx), its rows 0, 2 conditioned with the table rows of
// (by & 1, bx & 1) / (by & 1, ~bx & 1), its rows 1, 3 with those of the other row parity.
//
//   raw_lut_host PATTERN LUT.bin WINDOWS.bin OUT.bin
//
// LUT.bin: 1024 bytes, phase-major.  WINDOWS.bin: n windows of 16 bytes, row-major.  OUT.bin: per window and per parity pair
// (by & 1, bx & 1) = (0,0), (0,1), (1,0), (1,1) the four conditioned window rows as little-endian dwords, then the 16 bytes once more
// through condition1.  The table lives in a heap block of exactly 1024 bytes (the sanitizer build: any lookup outside it is an error).
// Prints "ok <n>".
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
    if (argc != 5) return 2;
    const int pattern = std::atoi(argv[1]);
    const std::vector<uint8_t> table = slurp(argv[2]), win = slurp(argv[3]);
    if (pattern < 0 || pattern > 3 || table.size() != 1024 || win.empty() || win.size() % 16) return 2;
    uint8_t* lut = static_cast<uint8_t*>(std::malloc(1024));
    if (!lut) return 3;
    std::memcpy(lut, table.data(), 1024);
    const size_t n = win.size() / 16;
    std::vector<uint32_t> out;
    out.reserve(n * 4 * 8);
    for (size_t i = 0; i < n; ++i) {
        uint32_t r[4];
        for (int k = 0; k < 4; ++k) std::memcpy(&r[k], &win[16 * i + 4 * k], 4);   // (little-endian host: byte c of a row is column c)
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                const uint8_t *ea = lut + ba::lut_row(pattern, py, px), *eb = lut + ba::lut_row(pattern, py, px ^ 1);
                const uint8_t *oa = lut + ba::lut_row(pattern, py ^ 1, px), *ob = lut + ba::lut_row(pattern, py ^ 1, px ^ 1);
                out.push_back(ba::condition4(r[0], ea, eb));
                out.push_back(ba::condition4(r[1], oa, ob));
                out.push_back(ba::condition4(r[2], ea, eb));
                out.push_back(ba::condition4(r[3], oa, ob));
                for (int k = 0; k < 4; ++k) {                 // the same, a byte at a time (the byte-wise row conversion)
                    uint32_t w = 0;
                    for (int c = 0; c < 4; ++c)
                        w |= ba::condition1(r[k] >> (8 * c), lut + ba::lut_row(pattern, py ^ (k & 1), px ^ (c & 1))) << (8 * c);
                    out.push_back(w);
                }
            }
    }
    std::free(lut);
    FILE* f = std::fopen(argv[4], "wb");
    if (!f) return 3;
    const size_t wrote = std::fwrite(out.data(), 4, out.size(), f);
    std::fclose(f);
    if (wrote != out.size()) return 3;
    std::printf("ok %zu\n", n);
    return 0;
}
