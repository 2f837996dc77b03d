// Host build of the raw Bayer arithmetic of lane_tracker_amd/csrc/bayer_arith.h, a stand-alone program for tests/test_bayer_cpu.py
// (built with the system C++ compiler, once plain and once with -fsanitize=address,undefined).
//
//   bayer_arith_host <pattern 0..3> <h> <w> <mosaic file: h * w bytes> <output file>
//
// For every bilinear sample (sy, sx) with sy in -3 .. h + 2 and sx in -3 .. w + 2 -- below 0, at 0, interior, at h - 2 / w - 2 and
// beyond -- it does what the undistortion walk does: the taps clamped to the frame as the walk hands them to a format (cy0, cy1, cx0,
// cx1), ba::place_axis on both axes, the four rows of the 4 x 4 window read with 4-byte copies out of a heap block of exactly h * w
// bytes (so that the address sanitizer sees a window that leaves the plane), ba::window_tap for the four taps.  The four pixels
// (R | G << 8 | B << 16) of every sample go to the output file, little endian, in that order; the Python test compares them with the
// NumPy restatement.  Checked here: the window starts where clamp(s - 1, 0, n - 4) says, from the clamped taps as from the raw
// coordinate; it lies inside the plane; every offset is 1 or 2; the row kernel's neighbourhood form (ba::demosaic with ba::phase at
// the clamped position) gives the same pixel as the window form; ba::input_run covers the windows of the rows it is asked for and
// ba::support_run the neighbourhoods.  Exit status 0 and one line "ok <samples>" when everything holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bayer_arith.h"

using namespace lt;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

int main(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: %s pattern h w mosaic out\n", argv[0]); return 2; }
    const int pattern = std::atoi(argv[1]), h = std::atoi(argv[2]), w = std::atoi(argv[3]);
    if (pattern < 0 || pattern > 3 || h < 4 || w < 4 || (h & 1) || (w & 1)) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    uint8_t* m = static_cast<uint8_t*>(std::malloc((size_t)h * w));     // exactly the plane
    if (!m) return 2;
    std::FILE* in = std::fopen(argv[4], "rb");
    if (!in || std::fread(m, 1, (size_t)h * w, in) != (size_t)h * w) { std::fprintf(stderr, "cannot read the mosaic\n"); return 2; }
    std::fclose(in);
    std::FILE* out = std::fopen(argv[5], "wb");
    if (!out) return 2;
    long samples = 0;
    for (int sy = -3; sy <= h + 2; ++sy) {
        for (int sx = -3; sx <= w + 2; ++sx) {
            // the walk: taps clamped to the frame
            const int cy0 = clampi(sy, 0, h - 1), cy1 = clampi(sy + 1, 0, h - 1), cx0 = clampi(sx, 0, w - 1), cx1 = clampi(sx + 1, 0, w - 1);
            const ba::Axis ay = ba::place_axis(cy0, cy1, h), ax = ba::place_axis(cx0, cx1, w);
            if (ay.origin != clampi(sy - 1, 0, h - 4) || ax.origin != clampi(sx - 1, 0, w - 4) || ay.origin != ba::win_origin(sy, h) ||
                ax.origin != ba::win_origin(sx, w)) {
                std::printf("origin: sample (%d, %d) of %dx%d -> (%d, %d)\n", sy, sx, w, h, ay.origin, ax.origin);
                return 1;
            }
            const int off[4] = {ay.o0, ay.o1, ax.o0, ax.o1};
            for (int o : off)
                if (o != 1 && o != 2) { std::printf("offset: sample (%d, %d) of %dx%d -> %d\n", sy, sx, w, h, o); return 1; }
            if (ay.origin + ay.o0 != ba::tap_pos(sy, h) || ay.origin + ay.o1 != ba::tap_pos(sy + 1, h) || ax.origin + ax.o0 != ba::tap_pos(sx, w) ||
                ax.origin + ax.o1 != ba::tap_pos(sx + 1, w)) {
                std::printf("tap position: sample (%d, %d) of %dx%d\n", sy, sx, w, h);
                return 1;
            }
            uint32_t r[4];
            for (int i = 0; i < 4; ++i) std::memcpy(&r[i], m + (size_t)(ay.origin + i) * w + ax.origin, 4);   // (little endian, as the device)
            const int oy[2] = {ay.o0, ay.o1}, py[2] = {ay.par0, ay.par1}, ox[2] = {ax.o0, ax.o1}, px[2] = {ax.par0, ax.par1};
            for (int j = 0; j < 2; ++j) {
                for (int i = 0; i < 2; ++i) {
                    const uint32_t v = ba::window_tap(r[0], r[1], r[2], r[3], oy[j], ox[i], ba::phase_of(pattern, py[j], px[i]));
                    // the row kernels' form: the neighbourhood of the clamped position, indexed directly
                    const int ty = ba::tap_pos(sy + j, h), tx = ba::tap_pos(sx + i, w);
                    const uint8_t *up = m + (size_t)(ty - 1) * w + tx, *mid = up + w, *dn = mid + w;
                    const uint32_t d = ba::demosaic(mid[0], (uint32_t)mid[-1] + mid[1], (uint32_t)up[0] + dn[0],
                                                    (uint32_t)up[-1] + up[1] + dn[-1] + dn[1], ba::phase(pattern, ty, tx));
                    if (v != d) { std::printf("forms: sample (%d, %d) tap (%d, %d) of %dx%d: %06x / %06x\n", sy, sx, j, i, w, h, v, d); return 1; }
                    if (std::fwrite(&v, 4, 1, out) != 1) return 2;
                }
            }
            ++samples;
        }
    }
    // the row runs: for every run of camera rows [r0, r1)
    for (int r0 = 0; r0 < h; ++r0) {
        for (int r1 = r0 + 1; r1 <= h; ++r1) {
            int s0, s1, a0, a1;
            ba::input_run(r0, r1, h, &s0, &s1);
            ba::support_run(r0, r1, h, &a0, &a1);
            bool ok = 0 <= s0 && s0 < s1 && s1 <= h && s1 - s0 >= 4 && 0 <= a0 && a0 < a1 && a1 <= h && s0 <= a0 && a1 <= s1;
            // a sample with a tap in [r0, r1): sy in r0 - 1 .. r1 - 1; its window's rows, clipped to what its in-image taps need
            for (int sy = r0 - 1; sy <= r1 - 1 && ok; ++sy) {
                const int by = ba::win_origin(sy, h);
                for (int t = sy; t <= sy + 1; ++t) {
                    if (t < r0 || t >= r1) continue;
                    const int ty = ba::tap_pos(t, h);
                    ok = ok && by <= ty - 1 && ty + 1 <= by + 3 && a0 <= ty - 1 && ty + 2 <= a1;
                }
                if (sy >= r0 && sy + 1 < r1) ok = ok && s0 <= by && by + 4 <= s1;      // both taps in the run: the whole window
            }
            if (!ok) { std::printf("runs: rows [%d, %d) of %d -> window rows [%d, %d), support rows [%d, %d)\n", r0, r1, h, s0, s1, a0, a1); return 1; }
        }
    }
    std::fclose(out);
    std::free(m);
    std::printf("ok %ld\n", samples);
    return 0;
}
