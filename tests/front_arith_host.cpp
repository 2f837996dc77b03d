// Host build of lane_tracker_amd/csrc/front_arith.h for tests/test_front_arith_cpu.py: the expressions k_frontend.hip runs,
// compiled with the system C++ compiler and called through ctypes.  (tests/front_arith_host.py builds it.)
#include <cstddef>
#include <cstdint>
#include <vector>

#include "front_arith.h"

using namespace lt;

extern "C" {

// taps: n sets of four RGBX dwords (top left, top right, bottom left, bottom right); out: [32 fy][32 fx][n][3] blended channels
// for every pair of fractions.  form 0: the 24-bit integer blend, 1: the fp32 blend; m: the taps inside the frame.
void fa_blend_all(int form, const uint32_t* taps, int n, unsigned m, uint8_t* out) {
    for (int fy = 0; fy < 32; ++fy)
        for (int fx = 0; fx < 32; ++fx) {
            const fa::WeightsI wi = fa::weights_i(fx, fy, m);
            const fa::Weights wf = fa::weights8(fx, fy, m);
            uint8_t* o = out + (size_t)(fy * 32 + fx) * n * 3;
            for (int k = 0; k < n; ++k) {
                const uint32_t* t = taps + 4 * (size_t)k;
                uint32_t v[3];
                if (form == 0) {
                    v[0] = fa::blend8<0>(t[0], t[1], t[2], t[3], wi);
                    v[1] = fa::blend8<1>(t[0], t[1], t[2], t[3], wi);
                    v[2] = fa::blend8<2>(t[0], t[1], t[2], t[3], wi);
                } else {
                    v[0] = fa::blend8<0>(t[0], t[1], t[2], t[3], wf);
                    v[1] = fa::blend8<1>(t[0], t[1], t[2], t[3], wf);
                    v[2] = fa::blend8<2>(t[0], t[1], t[2], t[3], wf);
                }
                for (int ch = 0; ch < 3; ++ch) o[3 * k + ch] = (uint8_t)fa::value_of(v[ch] & fa::ROW8_MASK);
            }
        }
}

int fa_lab_clamp_is_dead(int gamma_max, const int32_t* coeffs) { return fa::lab_clamp_is_dead(gamma_max, coeffs) ? 1 : 0; }

// Lab b of n RGB triples the way k_warp_split4 forms it: the folded tables, 8 x the channel as the row offset.
void fa_lab_b(const uint8_t* rgb, size_t n, const uint16_t* gamma_tab, const uint16_t* cbrt_tab, const int32_t* coeffs, int clamp,
              uint8_t* out) {
    std::vector<fa::YZ> yz(3 * 256);
    for (int ch = 0; ch < 3; ++ch)
        for (int v = 0; v < 256; ++v) yz[ch * 256 + v] = fa::yz_row(gamma_tab[v], coeffs, ch);
    auto row = [&](int ch, uint32_t off) {
        return *reinterpret_cast<const fa::YZ*>(reinterpret_cast<const char*>(&yz[ch * 256]) + off);
    };
    for (size_t i = 0; i < n; ++i) {
        const uint32_t r8 = 8u * rgb[3 * i], g8 = 8u * rgb[3 * i + 1], b8 = 8u * rgb[3 * i + 2];
        out[i] = (uint8_t)(clamp ? fa::lab_b_rows<true>(row(0, r8), row(1, g8), row(2, b8), cbrt_tab)
                                 : fa::lab_b_rows<false>(row(0, r8), row(1, g8), row(2, b8), cbrt_tab));
    }
}

}  // extern "C"
