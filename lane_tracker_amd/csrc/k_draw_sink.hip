// Annotated frames drawn on their way into the caller's surfaces (lt_overlay_run_to_surfaces), gfx950: the slots' dense RGB camera
// frames in; lane and text found per pixel as k_inplace.hip finds them (overlay_lane.h: the four taps against the polygon's row
// intervals, the glyph under the pixel) and applied by ia::draw_pixel -- lane, then text; out straight into the surfaces, RGB at
// their pitch or NV12 / I420 through sink_arith.h, chroma from the pixel at the even row and even column.  One pass over the frame
// where lt_overlay_run + lt_overlay_text + lt_overlay_store_device make three and keep a dense annotated frame between them.
//
//   k_draw_rows_to_surf<LAYOUT>      one thread owns two rows x 16 columns: 16-byte loads and stores (width a multiple of 16, every
//                                    base and pitch of the launch a multiple of 16 -- I420 chroma: 8)
//   k_draw_rows_to_surf_any<LAYOUT>  any geometry, byte accesses: one thread per 2 x 2 block (4:2:0) or per pixel (RGB)
//
// Tables per slot: frame blockIdx.z takes the inverse-warp tables of its own calibration set (SlotOv: the ids by value, the pair by
// scalar loads); a launch over one set is the same kernel with equal ids.  The table lookups and the four taps happen only in the
// union of the sets' lane rows [lane_r0, lane_r1), the glyph search only in the text's rows [text_r0, text_r1): both tests are
// uniform along a row, and every other row is a plain conversion.
//
// Every store lands inside a row's own bytes of its own plane (k_sink.hip's rule): nothing is written between rows or around planes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "lt_internal.h"
#include "overlay_lane.h"

namespace lt {
namespace {

struct DrawRows { int lane_r0, lane_r1, text_r0, text_r1; };

// pixel (x, y) of frame z as the annotated frame has it: px = R | G << 8 | B << 16 of the camera frame
__device__ __forceinline__ uint32_t drawn(uint32_t px, const OvTables& tb, const short2* __restrict__ sp, const InplaceLane& l,
                                          const InplaceText& t, bool lane_row, bool text_row, int z, int x, int y, int w) {
    int v = 0, a = 0;
    if (lane_row) {
        const int o = y * w + x;
        v = lane_value(sp, l.bh, l.bw, tb.oxy[2 * o], tb.oxy[2 * o + 1], tb.ofrac[o]);
    }
    if (text_row) a = text_alpha(t, z, x, y);
    return (v | a) ? ia::draw_pixel(px, v, a, l.alpha) : px;
}

// LAYOUT 0: RGB, 1: NV12, 2: I420.  Thread t: chroma row (row pair) cr = t / groups, columns [x0, x0 + 16).  RGB frames may have an
// odd height: the second row of the last pair is then not there.
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_draw_rows_to_surf(const uint8_t* __restrict__ rgb, size_t rgb_stride, SurfChunk ch,
                                                          const OvTables* __restrict__ sets, CalIds ids, InplaceLane l, InplaceText t,
                                                          DrawRows rows, sa::Rgb2Yuv k, int h, int w, int groups, int items) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= items) return;
    const int cr = i / groups, x0 = (i - cr * groups) * 16, z = (int)blockIdx.z;
    const SurfEntry& e = ch.e[z];
    const OvTables& tb = SlotOv{sets, &ids}.of(z);
    const short2* sp = reinterpret_cast<const short2*>(l.spans) + (size_t)z * l.span_stride_rows;
    const uint8_t* src = rgb + (size_t)z * rgb_stride;
    uint32_t cu[2] = {0u, 0u}, cv[2] = {0u, 0u};           // 8 U, 8 V
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * cr + dy;
        if (LAYOUT == 0 && y >= h) break;
        const uint4* s = reinterpret_cast<const uint4*>(src + ((size_t)y * w + x0) * 3);
        const uint4 q0 = s[0], q1 = s[1], q2 = s[2];
        const uint32_t d[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        uint32_t px[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t r = (d[(3 * j) >> 2] >> (8 * ((3 * j) & 3))) & 255u;
            const uint32_t g = (d[(3 * j + 1) >> 2] >> (8 * ((3 * j + 1) & 3))) & 255u;
            const uint32_t b = (d[(3 * j + 2) >> 2] >> (8 * ((3 * j + 2) & 3))) & 255u;
            px[j] = r | (g << 8) | (b << 16);
        }
        const bool lane_row = y >= rows.lane_r0 && y < rows.lane_r1, text_row = y >= rows.text_r0 && y < rows.text_r1;
        if (lane_row) {
            // the 16 pixels' table entries: 64 + 32 consecutive, aligned bytes
            const int o = y * w + x0;
            const uint4* pxy = reinterpret_cast<const uint4*>(tb.oxy + 2 * (size_t)o);
            const uint4* pfr = reinterpret_cast<const uint4*>(tb.ofrac + (size_t)o);
            const uint4 a0 = pxy[0], a1 = pxy[1], a2 = pxy[2], a3 = pxy[3], f0 = pfr[0], f1 = pfr[1];
            const uint32_t xy[16] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
            const uint32_t fr[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int v = lane_value(sp, l.bh, l.bw, (int16_t)(xy[j] & 0xffffu), (int16_t)(xy[j] >> 16), (int)((fr[j >> 1] >> (16 * (j & 1))) & 0xffffu));
                if (v) px[j] = ia::draw_pixel(px[j], v, 0, l.alpha);
            }
        }
        if (text_row) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int a = text_alpha(t, z, x0 + j, y);
                if (a) px[j] = ia::draw_pixel(px[j], 0, a, l.alpha);
            }
        }
        if constexpr (LAYOUT == 0) {
            uint32_t o[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) o[j] = 0u;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[(3 * j + c) >> 2] |= ((px[j] >> (8 * c)) & 255u) << (8 * ((3 * j + c) & 3));
            }
            uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(e.plane[0]) + (size_t)y * e.pitch + (size_t)x0 * 3);
            dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
            dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
            dst[2] = make_uint4(o[8], o[9], o[10], o[11]);
        } else {
            uint32_t yo[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int r = (int)(px[j] & 255u), g = (int)((px[j] >> 8) & 255u), b = (int)((px[j] >> 16) & 255u);
                yo[j >> 2] |= sa::luma(r, g, b, k) << (8 * (j & 3));
                if (dy == 0 && (j & 1) == 0) {
                    cu[j >> 3] |= sa::chroma_u(r, g, b, k) << (8 * ((j >> 1) & 3));
                    cv[j >> 3] |= sa::chroma_v(r, g, b, k) << (8 * ((j >> 1) & 3));
                }
            }
            *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(e.plane[0]) + (size_t)y * e.pitch + x0) = make_uint4(yo[0], yo[1], yo[2], yo[3]);
        }
    }
    if constexpr (LAYOUT == 1) {
        // U0 V0 U1 V1 ...: the bytes of cu and cv interleaved
        uint32_t p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t u2 = (cu[j >> 1] >> (16 * (j & 1))) & 0xffffu, v2 = (cv[j >> 1] >> (16 * (j & 1))) & 0xffffu;
            p[j] = (u2 & 255u) | ((v2 & 255u) << 8) | ((u2 >> 8) << 16) | ((v2 >> 8) << 24);
        }
        *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(e.plane[1]) + (size_t)cr * e.cpitch + x0) = make_uint4(p[0], p[1], p[2], p[3]);
    } else if constexpr (LAYOUT == 2) {
        const size_t co = (size_t)cr * e.cpitch + (size_t)(x0 >> 1);
        *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(e.plane[1]) + co) = make_uint2(cu[0], cu[1]);
        *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(e.plane[2]) + co) = make_uint2(cv[0], cv[1]);
    }
}

// the same for any width, pitch and alignment, byte accesses: RGB one pixel per thread (`groups` = w, items = h * w), 4:2:0 one
// thread per 2 x 2 block (`groups` = w / 2 per chroma row)
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_draw_rows_to_surf_any(const uint8_t* __restrict__ rgb, size_t rgb_stride, SurfChunk ch,
                                                              const OvTables* __restrict__ sets, CalIds ids, InplaceLane l, InplaceText t,
                                                              DrawRows rows, sa::Rgb2Yuv k, int h, int w, int groups, int items) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= items) return;
    const int row = i / groups, bx = i - row * groups, z = (int)blockIdx.z;
    const SurfEntry& e = ch.e[z];
    const OvTables& tb = SlotOv{sets, &ids}.of(z);
    const short2* sp = reinterpret_cast<const short2*>(l.spans) + (size_t)z * l.span_stride_rows;
    const uint8_t* src = rgb + (size_t)z * rgb_stride;
    uint8_t* p0 = reinterpret_cast<uint8_t*>(e.plane[0]);
    if constexpr (LAYOUT == 0) {
        const int y = row, x = bx;
        const uint8_t* s = src + ((size_t)y * w + x) * 3;
        const uint32_t px = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
        const uint32_t q = drawn(px, tb, sp, l, t, y >= rows.lane_r0 && y < rows.lane_r1, y >= rows.text_r0 && y < rows.text_r1, z, x, y, w);
        uint8_t* d = p0 + (size_t)y * e.pitch + 3 * (size_t)x;
        d[0] = (uint8_t)q;
        d[1] = (uint8_t)(q >> 8);
        d[2] = (uint8_t)(q >> 16);
    } else {
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * row + dy;
            const bool lane_row = y >= rows.lane_r0 && y < rows.lane_r1, text_row = y >= rows.text_r0 && y < rows.text_r1;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = 2 * bx + dx;
                const uint8_t* s = src + ((size_t)y * w + x) * 3;
                const uint32_t px = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
                const uint32_t q = drawn(px, tb, sp, l, t, lane_row, text_row, z, x, y, w);
                const int r = (int)(q & 255u), g = (int)((q >> 8) & 255u), b = (int)((q >> 16) & 255u);
                p0[(size_t)y * e.pitch + x] = (uint8_t)sa::luma(r, g, b, k);
                if (dy == 0 && dx == 0) {
                    const uint8_t u = (uint8_t)sa::chroma_u(r, g, b, k), v = (uint8_t)sa::chroma_v(r, g, b, k);
                    const size_t crow = (size_t)row * e.cpitch;
                    if constexpr (LAYOUT == 1) {
                        uint8_t* pc = reinterpret_cast<uint8_t*>(e.plane[1]) + crow + 2 * bx;
                        pc[0] = u;
                        pc[1] = v;
                    } else {
                        reinterpret_cast<uint8_t*>(e.plane[1])[crow + bx] = u;
                        reinterpret_cast<uint8_t*>(e.plane[2])[crow + bx] = v;
                    }
                }
            }
        }
    }
}

}  // namespace

int launch_draw_to_surfaces(hipStream_t s, int layout, const uint8_t* rgb, size_t rgb_stride, int h, int w, const SurfEntry* entries,
                            int n, const OvTables* sets, const uint8_t* ids, InplaceLane l, InplaceText t, int lane_r0, int lane_r1,
                            const int32_t* coeffs) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    const sa::Rgb2Yuv k = layout != 0 ? sa::coef_of(coeffs) : sa::Rgb2Yuv{};
    DrawRows rows{std::max(lane_r0, 0), std::min(lane_r1, h), 0, 0};
    if (t.nl > 0) {
        rows.text_r0 = std::max(t.y0, 0);
        rows.text_r1 = std::min(t.y0 + (t.nl - 1) * t.step + t.gh, h);
    }
    int launches = 0;
    for (int at = 0; at < n; at += SurfChunk::N, ++launches) {
        const int m = std::min(n - at, (int)SurfChunk::N);
        SurfChunk ch{};
        std::copy(entries + at, entries + at + m, ch.e);
        const CalIds ci = pack_cal_ids(ids + at, m);
        const uint8_t* src = rgb + (size_t)at * rgb_stride;
        const InplaceDraw d = advanced(l, t, at);
        size_t bits = rgb_stride | (size_t)(uintptr_t)src, cbits = 0;   // every base and pitch of the launch a multiple of 16 (I420 chroma: 8)?
        for (int j = 0; j < m; ++j) {
            bits |= (size_t)ch.e[j].plane[0] | (size_t)ch.e[j].pitch;
            if (layout == 1) bits |= (size_t)ch.e[j].plane[1] | (size_t)ch.e[j].cpitch;
            if (layout == 2) cbits |= (size_t)ch.e[j].plane[1] | (size_t)ch.e[j].plane[2] | (size_t)ch.e[j].cpitch;
        }
        if ((w & 15) == 0 && (bits & 15) == 0 && (cbits & 7) == 0) {
            const int groups = w / 16, items = ((h + 1) / 2) * groups;
            auto kern = layout == 0 ? k_draw_rows_to_surf<0> : layout == 1 ? k_draw_rows_to_surf<1> : k_draw_rows_to_surf<2>;
            hipLaunchKernelGGL(kern, dim3((unsigned)((items + 255) / 256), 1, (unsigned)m), dim3(256), 0, s, src, rgb_stride, ch, sets, ci, d.l, d.t,
                               rows, k, h, w, groups, items);
        } else {
            const int groups = layout == 0 ? w : w / 2, items = (layout == 0 ? h : h / 2) * groups;
            auto kern = layout == 0 ? k_draw_rows_to_surf_any<0> : layout == 1 ? k_draw_rows_to_surf_any<1> : k_draw_rows_to_surf_any<2>;
            hipLaunchKernelGGL(kern, dim3((unsigned)((items + 255) / 256), 1, (unsigned)m), dim3(256), 0, s, src, rgb_stride, ch, sets, ci, d.l, d.t,
                               rows, k, h, w, groups, items);
        }
    }
    return launches;
}

}  // namespace lt
