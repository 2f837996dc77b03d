// Host build of the packed 4:2:2 position arithmetic of lane_tracker_amd/csrc/yuv_arith.h, a stand-alone program for
// tests/test_yuv422_cpu.py (built with the system C++ compiler, once plain and once with -fsanitize=address,undefined).
//
// For every even width 4 .. 18, every leftmost tap column cxl in 0 .. W - 2, both byte orders and both taps: the window and the bit
// positions the header computes select the same Y, U, V as direct indexing of a random row, and the converted pixel is
// yuv_pixel(Y, yuv_chroma(U, V)).  The window never starts before its row and ends at byte 4 * min(cxl >> 1, W / 2 - 2) + 8, which
// is never behind the row's last byte: every row lives in a heap block of exactly 2 W bytes, so that the
// address sanitizer sees an overrun.  Exit status 0 and one line "ok <checks>" when everything holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "yuv_arith.h"

using namespace lt;

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

int main() {
    const YuvCoef k{1220542, 1673527, -852492, -409993, 2116026};
    long checks = 0;
    for (int order = 0; order < 2; ++order) {
        for (int w = 4; w <= 18; w += 2) {
            uint8_t* row = static_cast<uint8_t*>(std::malloc((size_t)2 * w));
            if (!row) return 2;
            for (int rep = 0; rep < 8; ++rep) {
                for (int i = 0; i < 2 * w; ++i) row[i] = (uint8_t)(rnd() >> 11);
                if (rep == 0) std::memset(row, 0, (size_t)2 * w);          // the extremes: every clamp of the conversion
                if (rep == 1) std::memset(row, 255, (size_t)2 * w);
                for (int cxl = 0; cxl <= w - 2; ++cxl) {
                    const int mp = ya::win422_mp(cxl, w / 2 - 2), col = ya::win422_col(mp);
                    const int want_end = 4 * ((cxl >> 1) < w / 2 - 2 ? (cxl >> 1) : w / 2 - 2) + 8;
                    if (col < 0 || col + 8 != want_end || col + 8 > 2 * w) {
                        std::printf("window: order %d w %d cxl %d -> bytes [%d, %d) of %d\n", order, w, cxl, col, col + 8, 2 * w);
                        return 1;
                    }
                    uint32_t win[2];
                    std::memcpy(win, row + col, 8);                        // the one window of the tap row (little endian, as the device)
                    for (int cx = cxl; cx <= cxl + 1; ++cx) {
                        const int dw = ya::win422_dword(cx, mp);
                        if (dw != 0 && dw != 1) { std::printf("dword: order %d w %d cxl %d cx %d -> %d\n", order, w, cxl, cx, dw); return 1; }
                        const uint32_t d = win[dw];
                        const int ysh = ya::ysh422(order, cx);
                        const int y = (int)((d >> ysh) & 255u), u = (int)((d >> ya::ush422(order)) & 255u), v = (int)((d >> ya::vsh422(order)) & 255u);
                        // direct indexing: macropixel cx >> 1 of the row; YUY2: Y0 U Y1 V, UYVY: U Y0 V Y1
                        const uint8_t* m = row + 4 * (cx >> 1);
                        const int wy = order == 0 ? m[2 * (cx & 1)] : m[2 * (cx & 1) + 1], wu = order == 0 ? m[1] : m[0], wv = order == 0 ? m[3] : m[2];
                        if (y != wy || u != wu || v != wv) {
                            std::printf("samples: order %d w %d cxl %d cx %d -> (%d %d %d), want (%d %d %d)\n", order, w, cxl, cx, y, u, v, wy, wu, wv);
                            return 1;
                        }
                        if (ya::yuv422_pixel(d, order, ysh, k) != ya::yuv_pixel(wy, ya::yuv_chroma(wu, wv, k), k)) {
                            std::printf("pixel: order %d w %d cxl %d cx %d\n", order, w, cxl, cx);
                            return 1;
                        }
                        ++checks;
                    }
                }
            }
            std::free(row);
        }
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
