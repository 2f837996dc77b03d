// csrc/mipi_arith.h on the host: the window extraction of the walk (unpack_of + samples4), the 16 columns of the row conversion's wide
// body (group4) and the site-wise access (site_at), each against the plain unpack of the definitions (the packer below is a restatement of
// them, site by site).  For both packings: every window origin bx in 0 .. W - 4 at W = 64, 66 (RAW12 only: RAW10 needs W % 4 == 0) and 68,
// every alignment 0 .. 3 of the row's first byte, random rows, a row of only low bits and a row of only high bits.  The window is fetched
// as the device fetches it: the three aligned dwords that hold the bytes from the window's first byte, shifted into place.
// Exit status 0 and "ok <checks>" on stdout, or a message on stderr and status 1.  Built by tests/test_raw_packed_cpu.py, plain and under
// ASan / UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mipi_arith.h"

using namespace lt;

// the definitions, site by site
static void pack_row(int pack, const std::vector<uint16_t>& s, uint8_t* row) {
    const int w = (int)s.size();
    if (pack == ma::PACK10) {
        for (int g = 0; g < w / 4; ++g) {
            uint32_t low = 0;
            for (int i = 0; i < 4; ++i) {
                row[5 * g + i] = (uint8_t)(s[4 * g + i] >> 2);
                low |= (uint32_t)(s[4 * g + i] & 3) << (2 * i);
            }
            row[5 * g + 4] = (uint8_t)low;
        }
    } else {
        for (int g = 0; g < w / 2; ++g) {
            row[3 * g] = (uint8_t)(s[2 * g] >> 4);
            row[3 * g + 1] = (uint8_t)(s[2 * g + 1] >> 4);
            row[3 * g + 2] = (uint8_t)((s[2 * g] & 15) | ((s[2 * g + 1] & 15) << 4));
        }
    }
}

// v_alignbyte_b32
static uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3u))); }
static uint32_t dword_at(const uint8_t* p) {
    uint32_t v;
    std::memcpy(&v, p, 4);
    return v;
}

static long checks = 0;
static int fail(const char* what, int pack, int w, int align, int x, unsigned got, unsigned want) {
    std::fprintf(stderr, "%s: pack %d w %d align %d site %d: got %u, want %u\n", what, pack, w, align, x, got, want);
    return 1;
}

template <int PACK>
static int check_row(const std::vector<uint16_t>& s, int align) {
    const int w = (int)s.size(), rb = ma::row_bytes(PACK, w);
    // the row at byte `align` of a block of whole dwords with three dwords of slack behind it, as a buffer resource returns them: zeros
    std::vector<uint32_t> block((size_t)(align + rb + 3) / 4 + 3, 0u);
    uint8_t* base = reinterpret_cast<uint8_t*>(block.data());
    uint8_t* row = base + align;
    pack_row(PACK, s, row);
    if (rb != (PACK == ma::PACK10 ? 5 * w / 4 : 3 * w / 2)) return fail("row_bytes", PACK, w, align, 0, (unsigned)rb, 0);
    for (int x = 0; x < w; ++x, ++checks)
        if (ma::site_at(PACK, row, x) != s[(size_t)x]) return fail("site_at", PACK, w, align, x, ma::site_at(PACK, row, x), s[(size_t)x]);
    for (int bx = 0; bx + 4 <= w; ++bx) {
        const int first = ma::first_byte(PACK, bx);
        if (first != (PACK == ma::PACK10 ? 5 * (bx >> 2) + (bx & 3) : 3 * (bx >> 1) + (bx & 1))) return fail("first_byte", PACK, w, align, bx, (unsigned)first, 0);
        // the window never needs a byte behind its row: the last byte it may use is the row's last
        const uint32_t off = (uint32_t)(align + first);
        const uint8_t* a = base + (off & ~3u);
        const uint32_t d0 = dword_at(a), d1 = dword_at(a + 4), d2 = dword_at(a + 8);
        const uint32_t w0 = alignbyte(d1, d0, off), w1 = alignbyte(d2, d1, off), w2 = PACK == ma::PACK10 ? alignbyte(0u, d2, off) : 0u;
        const ma::Unpack u = ma::unpack_of(PACK, bx);
        uint32_t lo, hi;
        ma::samples4<PACK>(u, w0, w1, w2, lo, hi);
        const unsigned got[4] = {lo & 0xffffu, lo >> 16, hi & 0xffffu, hi >> 16};
        for (int k = 0; k < 4; ++k, ++checks)
            if (got[k] != s[(size_t)(bx + k)]) return fail("samples4", PACK, w, align, bx + k, got[k], s[(size_t)(bx + k)]);
        // every byte the extraction uses lies inside the row: a window whose other bytes are garbage gives the same samples
        const int used = PACK == ma::PACK10 ? 9 : 8, avail = rb - first < used ? rb - first : used;
        uint32_t g[3] = {w0, w1, w2};
        for (int b = avail; b < 12; ++b) reinterpret_cast<uint8_t*>(g)[b] ^= 0xa5;
        if (PACK == ma::PACK12) g[2] = 0xdeadbeefu;
        uint32_t lo2, hi2;
        ma::samples4<PACK>(u, g[0], g[1], g[2], lo2, hi2);
        ++checks;
        if (lo2 != lo || hi2 != hi) return fail("samples4 reads outside its span", PACK, w, align, bx, lo2, lo);
    }
    if (w % 16 == 0 && (align & 3) == 0)
        for (int x0 = 0; x0 < w; x0 += 16) {
            uint32_t m[6] = {};
            std::memcpy(m, row + ma::first_byte(PACK, x0), PACK == ma::PACK10 ? 20 : 24);
            for (int j = 0; j < 4; ++j) {
                uint32_t lo, hi;
                ma::group4<PACK>(m, j, lo, hi);
                const unsigned got[4] = {lo & 0xffffu, lo >> 16, hi & 0xffffu, hi >> 16};
                for (int k = 0; k < 4; ++k, ++checks)
                    if (got[k] != s[(size_t)(x0 + 4 * j + k)]) return fail("group4", PACK, w, align, x0 + 4 * j + k, got[k], s[(size_t)(x0 + 4 * j + k)]);
            }
        }
    return 0;
}

template <int PACK>
static int check_pack() {
    const unsigned smax = (1u << ma::bits_of(PACK)) - 1u, lowmask = PACK == ma::PACK10 ? 3u : 15u;
    uint32_t rng = 0x9e3779b9u + (uint32_t)PACK;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    const int widths[3] = {64, 66, 68};
    for (int w : widths) {
        if (PACK == ma::PACK10 && w % 4) continue;
        for (int align = 0; align < 4; ++align) {
            std::vector<uint16_t> s((size_t)w);
            for (int rep = 0; rep < 4; ++rep) {
                for (auto& v : s) v = (uint16_t)(next() & smax);
                if (check_row<PACK>(s, align)) return 1;
            }
            for (auto& v : s) v = (uint16_t)(next() & lowmask);                     // only low bits
            if (check_row<PACK>(s, align)) return 1;
            for (auto& v : s) v = (uint16_t)(next() & smax & ~lowmask);             // only high bits
            if (check_row<PACK>(s, align)) return 1;
            for (int x = 0; x < w; ++x) s[(size_t)x] = (uint16_t)(((unsigned)x * 37u + 1u) & lowmask) ;   // low bits that follow x % 4
            if (check_row<PACK>(s, align)) return 1;
            for (auto& v : s) v = (uint16_t)smax;
            if (check_row<PACK>(s, align)) return 1;
        }
    }
    return 0;
}

int main() {
    if (check_pack<ma::PACK10>() || check_pack<ma::PACK12>()) return 1;
    std::printf("ok %ld\n", checks);
    return 0;
}
