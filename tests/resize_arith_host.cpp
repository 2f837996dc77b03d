// Host build of lane_tracker_amd/csrc/resize_arith.h -- the taps, the blend and the input-row formula of the input-size path -- a
// stand-alone program for tests/test_input_size_cpu.py (built with the system C++ compiler, once plain and once with
// -fsanitize=address,undefined).
//
//   resize_arith_host <taps file> <images file>
// taps file (int32): pairs; per pair: src_len, dst_len, then dst_len x (tap0, tap1, c0, c1) as utils._resize_taps gives them.
//   Every entry must equal resize_tap(); c0 + c1 == 2048; the taps lie inside the axis and are monotone; input_run() of every run
//   [a, b) of a pair of up to 40 samples (of 64 spread runs of a longer one) equals a brute-force scan of the taps.
// images file: int32 cases; per case: sh, sw, dh, dw (int32), the source image (sh x sw x 3 bytes) and oracle.resize_linear's
//   result (dh x dw x 3 bytes).  Every image is resized the way k_resize_rows does it: pack_column's window position and tap
//   selectors, an 8-byte window per tap row that reads zeros behind the frame's last byte (the buffer resource's range check; the
//   source lives in a heap block of exactly its size, so that the address sanitizer sees anything else), resize_blend per channel.
//   The bytes the taps select must lie inside their row.
// Exit status 0 and one line "ok <tap entries> <runs> <pixels>" when everything holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "resize_arith.h"

using namespace lt;

static bool read_all(const char* path, std::vector<uint8_t>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)n);
    const bool ok = n == 0 || std::fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    std::fclose(f);
    return ok;
}

static int32_t i32_at(const std::vector<uint8_t>& b, size_t& pos) {
    if (pos + 4 > b.size()) { std::printf("truncated file\n"); std::exit(2); }
    int32_t v;
    std::memcpy(&v, b.data() + pos, 4);
    pos += 4;
    return v;
}

static bool check_run(int src, int dst, int a, int b, const std::vector<rz::Tap>& t) {
    int lo = 1 << 30, hi = -1;
    for (int i = a; i < b; ++i) {
        if (t[(size_t)i].tap0 < lo) lo = t[(size_t)i].tap0;
        if (t[(size_t)i].tap1 + 1 > hi) hi = t[(size_t)i].tap1 + 1;
    }
    int s0, s1;
    rz::input_run(src, dst, a, b, &s0, &s1);
    if (b <= a) return s0 == s1;
    if (s0 != lo || s1 != hi) {
        std::printf("input_run: %d -> %d, [%d, %d): [%d, %d), scan [%d, %d)\n", src, dst, a, b, s0, s1, lo, hi);
        return false;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::vector<uint8_t> file;
    long entries = 0, runs = 0, pixels = 0;

    if (!read_all(argv[1], file)) return 2;
    size_t pos = 0;
    const int pairs = i32_at(file, pos);
    for (int p = 0; p < pairs; ++p) {
        const int src = i32_at(file, pos), dst = i32_at(file, pos);
        std::vector<rz::Tap> taps((size_t)dst);
        for (int i = 0; i < dst; ++i) {
            const int32_t want[4] = {i32_at(file, pos), i32_at(file, pos), i32_at(file, pos), i32_at(file, pos)};
            const rz::Tap t = rz::resize_tap(src, dst, i);
            if (t.tap0 != want[0] || t.tap1 != want[1] || t.c0 != want[2] || t.c1 != want[3]) {
                std::printf("tap: %d -> %d, index %d: (%d, %d, %d, %d), table (%d, %d, %d, %d)\n", src, dst, i, t.tap0, t.tap1, t.c0, t.c1,
                            want[0], want[1], want[2], want[3]);
                return 1;
            }
            const bool adjacent = t.tap1 == t.tap0 + 1 || (t.tap1 == t.tap0 && t.c1 == 0);
            if (t.c0 + t.c1 != 2048 || t.c0 < 0 || t.c1 < 0 || t.tap0 < 0 || t.tap1 >= src || !adjacent ||
                (i > 0 && t.tap0 < taps[(size_t)i - 1].tap0)) {
                std::printf("tap: %d -> %d, index %d: (%d, %d, %d, %d) breaks an invariant\n", src, dst, i, t.tap0, t.tap1, t.c0, t.c1);
                return 1;
            }
            taps[(size_t)i] = t;
            ++entries;
        }
        if (dst <= 40) {
            for (int a = 0; a <= dst; ++a)
                for (int b = a; b <= dst; ++b, ++runs)
                    if (!check_run(src, dst, a, b, taps)) return 1;
        } else {
            for (int k = 0; k < 64; ++k, ++runs) {
                const int a = (int)((long long)dst * k / 64), b = a + 1 + (int)((long long)(dst - a - 1) * ((k * 37) % 64) / 64);
                if (!check_run(src, dst, a, b, taps)) return 1;
            }
        }
    }

    if (!read_all(argv[2], file)) return 2;
    pos = 0;
    const int cases = i32_at(file, pos);
    for (int q = 0; q < cases; ++q) {
        const int sh = i32_at(file, pos), sw = i32_at(file, pos), dh = i32_at(file, pos), dw = i32_at(file, pos);
        const size_t nsrc = (size_t)sh * sw * 3, ndst = (size_t)dh * dw * 3;
        if (pos + nsrc + ndst > file.size()) return 2;
        uint8_t* src = static_cast<uint8_t*>(std::malloc(nsrc));            // exactly the frame: nothing behind it may be read
        if (!src) return 2;
        std::memcpy(src, file.data() + pos, nsrc);
        const uint8_t* want = file.data() + pos + nsrc;
        pos += nsrc + ndst;
        const size_t records = (nsrc + 3) & ~(size_t)3;                     // the buffer resource: whole dwords of the frame
        for (int y = 0; y < dh; ++y) {
            const rz::Tap ty = rz::resize_tap(sh, dh, y);
            for (int x = 0; x < dw; ++x) {
                uint32_t cw[2];
                rz::pack_column(rz::resize_tap(sw, dw, x), sw, cw);
                const uint32_t col = cw[0] & 0xffffu, d0 = (cw[0] >> 16) & 1u, d1 = (cw[0] >> 17) & 1u, a0 = cw[1] & 0xffffu, a1 = cw[1] >> 16;
                if (col + 3 * d0 + 3 > (uint32_t)sw * 3 || (a1 != 0 && col + 3 * d1 + 3 > (uint32_t)sw * 3)) {
                    std::printf("window: %dx%d -> %dx%d, column %d: taps at bytes %u, %u of a row of %d\n", sw, sh, dw, dh, x, col + 3 * d0,
                                col + 3 * d1, sw * 3);
                    return 1;
                }
                uint8_t win[2][8];
                const int32_t rows[2] = {ty.tap0, ty.tap1};
                for (int r = 0; r < 2; ++r)
                    for (int i = 0; i < 8; ++i) {
                        const size_t at = (size_t)rows[r] * sw * 3 + col + (size_t)i;
                        if (at >= records) { win[r][i] = 0; continue; }       // the range check's zeros
                        // (bytes of the last dword behind the frame are the context's padding: never a tap, see the check above)
                        win[r][i] = at < nsrc ? src[at] : (uint8_t)0xEE;
                    }
                for (int ch = 0; ch < 3; ++ch, ++pixels) {
                    const uint32_t got = rz::resize_blend(win[0][3 * d0 + ch], win[0][3 * d1 + ch], win[1][3 * d0 + ch], win[1][3 * d1 + ch], a0, a1,
                                                          (uint32_t)ty.c0, (uint32_t)ty.c1);
                    if (got != want[((size_t)y * dw + x) * 3 + ch]) {
                        std::printf("blend: %dx%d -> %dx%d at (%d, %d, %d): %u, oracle %u\n", sw, sh, dw, dh, y, x, ch, got,
                                    (unsigned)want[((size_t)y * dw + x) * 3 + ch]);
                        return 1;
                    }
                }
            }
        }
        std::free(src);
    }
    std::printf("ok %ld %ld %ld\n", entries, runs, pixels);
    return 0;
}
