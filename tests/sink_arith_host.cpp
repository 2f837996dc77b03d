// Host build of lane_tracker_amd/csrc/sink_arith.h for tests/test_sink_arith_cpu.py: the expressions k_sink.hip runs, compiled
// with the system C++ compiler and called through ctypes.
#include <cstddef>
#include <cstdint>

#include "sink_arith.h"

using namespace lt;

extern "C" {

// n RGB triples (interleaved) -> n (Y, U, V) triples (interleaved) with coeffs[8]
void sa_forward(const uint8_t* rgb, size_t n, const int32_t* coeffs, uint8_t* yuv) {
    const sa::Rgb2Yuv k = sa::coef_of(coeffs);
    for (size_t i = 0; i < n; ++i) {
        const int r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
        yuv[3 * i] = (uint8_t)sa::luma(r, g, b, k);
        yuv[3 * i + 1] = (uint8_t)sa::chroma_u(r, g, b, k);
        yuv[3 * i + 2] = (uint8_t)sa::chroma_v(r, g, b, k);
    }
}

int sa_coeffs_ok(const int32_t* coeffs) { return sa::coeffs_ok(coeffs) ? 1 : 0; }

void sa_matrix(int which, int32_t* out) {
    for (int i = 0; i < 8; ++i) out[i] = which == 0 ? sa::BT601[i] : sa::BT709[i];
}

}  // extern "C"
