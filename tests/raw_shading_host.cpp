// The lens-shading expressions of csrc/shade_arith.h on the host, as k_shade_expand, the raw walks and the raw row conversions with a map (STAGES bit 2) of
// k_frontend.hip run them: the expansion of a mesh into the gain plane (gain_at), one sample (shade, and shade_plain: the definition as it
// is written), and the four-site forms with the table lookup behind them (shade_condition4 / shade_condition4w).
//
//   raw_shading_host IN.bin OUT.bin
//
// IN.bin, little-endian: int32 h, w, mw, mh, pattern, bits; int32 black[4]; uint16 mesh[4][mh][mw]; uint16 frame[h][w] (8 bits: the byte
// in a word; 10 / 12 bits: any word, the bits above the sample are ignored); uint8 table[4][1 << bits].  w is a multiple of 4.
// OUT.bin: uint16 plane[h][w]; uint16 shaded[h][w]; uint8 looked_up[h][w] = table[phase][shaded].  Mesh, table and frame live in heap blocks
// of exactly their size (the sanitizer build: a node, a lookup or a site outside them is an error; so is a signed overflow of a product).
// Exit code 4: shade and shade_plain, or the four-site form and the single one, disagree.  Prints "ok <sites>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bayer_arith.h"
#include "shade_arith.h"

namespace ba = lt::ba;
namespace sa = lt::sa;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[10];
    if (std::fread(head, sizeof head, 1, f) != 1) return 2;
    const int h = head[0], w = head[1], mw = head[2], mh = head[3], pattern = head[4], bits = head[5];
    const int32_t* black = head + 6;
    if (h < 2 || w < 4 || (w & 3) || mw < sa::MESH_MIN || mw > sa::MESH_MAX || mh < sa::MESH_MIN || mh > sa::MESH_MAX || (bits != 8 && bits != 10 && bits != 12)) return 2;
    const size_t nodes = (size_t)4 * mh * mw, px = (size_t)h * w, entries = (size_t)1 << bits;
    uint16_t* mesh = static_cast<uint16_t*>(std::malloc(nodes * 2));
    uint16_t* frame = static_cast<uint16_t*>(std::malloc(px * 2));
    uint8_t* table = static_cast<uint8_t*>(std::malloc(4 * entries));
    if (!mesh || !frame || !table) return 3;
    if (std::fread(mesh, 2, nodes, f) != nodes || std::fread(frame, 2, px, f) != px || std::fread(table, 1, 4 * entries, f) != 4 * entries) return 2;
    std::fclose(f);
    const int smax = (1 << bits) - 1;
    const uint32_t mask = (uint32_t)smax;
    std::vector<uint16_t> plane(px), shaded(px);
    std::vector<uint8_t> looked(px);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int p = ba::phase(pattern, y, x);
            const uint32_t g = sa::gain_at(mesh + (size_t)p * mh * mw, mw, mh, y, x, h, w);
            if (g > 65535u) return 4;
            plane[(size_t)y * w + x] = (uint16_t)g;
            const uint32_t s = frame[(size_t)y * w + x] & mask;
            const uint32_t v = sa::shade(s, black[p], sa::round_term(black[p]), g, smax);
            if (v != sa::shade_plain(s, black[p], g, smax)) return 4;
            shaded[(size_t)y * w + x] = (uint16_t)v;
        }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; x += 4) {
            const size_t at = (size_t)y * w + x;
            const uint8_t *rowa = table + entries * ba::phase(pattern, y, x), *rowb = table + entries * ba::phase(pattern, y, x + 1);
            const sa::Black2 k = sa::black2(black[ba::phase(pattern, y, x)], black[ba::phase(pattern, y, x + 1)]);
            const uint32_t glo = (uint32_t)plane[at] | ((uint32_t)plane[at + 1] << 16), ghi = (uint32_t)plane[at + 2] | ((uint32_t)plane[at + 3] << 16);
            uint32_t c;
            if (bits == 8) {
                const uint32_t wd = (frame[at] & 255u) | ((frame[at + 1] & 255u) << 8) | ((frame[at + 2] & 255u) << 16) | ((uint32_t)(frame[at + 3] & 255u) << 24);
                c = sa::shade_condition4(wd, glo, ghi, k, rowa, rowb);
            } else {
                const uint32_t lo = (uint32_t)frame[at] | ((uint32_t)frame[at + 1] << 16), hi = (uint32_t)frame[at + 2] | ((uint32_t)frame[at + 3] << 16);
                c = sa::shade_condition4w(lo, hi, glo, ghi, k, rowa, rowb, mask);
            }
            for (int i = 0; i < 4; ++i) {
                looked[at + i] = (uint8_t)(c >> (8 * i));
                if (looked[at + i] != (table + entries * ba::phase(pattern, y, x + i))[shaded[at + i]]) return 4;
            }
        }
    std::free(mesh);
    std::free(frame);
    std::free(table);
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    const bool ok = std::fwrite(plane.data(), 2, px, f) == px && std::fwrite(shaded.data(), 2, px, f) == px && std::fwrite(looked.data(), 1, px, f) == px;
    std::fclose(f);
    if (!ok) return 3;
    std::printf("ok %zu\n", px);
    return 0;
}
