// The colour stage's expression of csrc/bayer_arith.h (color_px: colour-correction matrix in Q10, clamp, output curve) on the host, as
// the raw walks and row conversions of k_frontend.hip (k_raw_walk_rows, k_raw_rows_rgb with STAGES bit 1) run it on every demosaiced pixel.
//
//   raw_color_host IN.bin OUT.bin N
//
// IN.bin: the matrix, nine little-endian int16, row-major; the curve, 256 bytes; N pixels of three bytes R, G, B.  OUT.bin: N pixels of
// three bytes.  The curve lives in a heap block of exactly 256 bytes (the sanitizer build: a lookup outside it -- a clamp that lets a
// value through -- is an error; so is a signed overflow of the sum).  Prints "ok <n>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bayer_arith.h"

namespace ba = lt::ba;

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const size_t n = (size_t)std::atol(argv[3]);
    std::vector<uint8_t> in(18 + 256 + 3 * n);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const size_t got = std::fread(in.data(), 1, in.size(), f);
    std::fclose(f);
    if (got != in.size() || n == 0) return 2;
    int m[9];
    for (int i = 0; i < 9; ++i) {
        int16_t v;
        std::memcpy(&v, &in[2 * i], 2);                           // (little-endian host)
        m[i] = v;
    }
    uint8_t* curve = static_cast<uint8_t*>(std::malloc(256));
    if (!curve) return 3;
    std::memcpy(curve, &in[18], 256);
    std::vector<uint8_t> out(3 * n);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* p = &in[18 + 256 + 3 * i];
        const uint32_t v = ba::color_px((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16), m, curve);
        out[3 * i] = (uint8_t)(v & 255u), out[3 * i + 1] = (uint8_t)((v >> 8) & 255u), out[3 * i + 2] = (uint8_t)(v >> 16);
    }
    std::free(curve);
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    const size_t wrote = std::fwrite(out.data(), 1, out.size(), f);
    std::fclose(f);
    if (wrote != out.size()) return 3;
    std::printf("ok %zu\n", n);
    return 0;
}
