// Lane and text drawn INTO the camera surfaces the caller attached (lt_overlay_run_inplace), gfx950.
//
// An annotated frame differs from its camera frame only where the lane polygon lands and under the text lines.  These kernels
// visit the rows either can reach -- two runs of rows, or one where they meet -- read the surface where it lies, and store only
// what changed: no copy of the frame into the slot, no dense annotated frame, no second surface.
//
//   k_inplace_rgb4    RGB surfaces, four pixels (three dwords) per thread: width, bases and pitches multiples of 4
//   k_inplace_rgb     RGB surfaces of any geometry, one pixel per thread, byte accesses
//   k_inplace_420     NV12 / I420, one thread per 2 x 2 block (byte accesses) or per four blocks side by side (8-byte luma rows;
//                     width, luma bases and pitches multiples of 8, chroma of 8 (NV12) / 4 (I420))
//   k_inplace_*_cal   the same bodies for a launch whose slots mix calibration sets: frame blockIdx.z with the inverse-warp tables
//                     of its own set (overlay_lane.h: SlotOv), CalIds::N slots per launch
//
// Lane and text of a pixel are found FIRST (overlay_lane.h: the four taps against the polygon's row intervals; the glyph under the
// pixel from the slot's list of character positions); a thread none of whose pixels is reached loads and stores nothing.  A 4:2:0
// block that is reached is converted to RGB once, drawn on -- lane, then text -- and converted back once (inplace_arith.h); of its
// six bytes only those whose RGB pixel changed are replaced.  Every byte of a surface has ONE thread that may touch it, and that
// thread reads it before it writes it, so the launch has no hazard within itself; the surfaces reach it through the context's
// per-slot table (frame blockIdx.z is entry blockIdx.z from the launch's first slot), like the undistortion's table form.
//
// Every store lands inside a row's own bytes of its own plane: nothing is written between rows or around planes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "lt_internal.h"
#include "overlay_lane.h"

namespace lt {
namespace {

__device__ __forceinline__ int row_of(const InplaceRows& r, int i) { return i < r.an ? r.a0 + i : r.b0 + (i - r.an); }

// the lane's value at camera pixel o = y * w + x of frame z
__device__ __forceinline__ int lane_at(const InplaceLane& l, const short2* __restrict__ sp, int o) {
    return lane_value(sp, l.bh, l.bw, l.oxy[2 * o], l.oxy[2 * o + 1], l.ofrac[o]);
}

__device__ __forceinline__ void inplace_rgb_body(const SurfEntry* __restrict__ tab, const InplaceRows& rows, const InplaceLane& l,
                                                 const InplaceText& t, int w, int items) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= items) return;
    const int ri = i / w, x = i - ri * w, y = row_of(rows, ri), z = (int)blockIdx.z;
    const int v = lane_at(l, reinterpret_cast<const short2*>(l.spans) + (size_t)z * l.span_stride_rows, y * w + x);
    const int a = text_alpha(t, z, x, y);
    if (!(v | a)) return;
    const SurfEntry& e = tab[z];
    uint8_t* p = reinterpret_cast<uint8_t*>(e.plane[0]) + (size_t)y * e.pitch + 3 * x;
    const uint32_t px = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    const uint32_t q = ia::draw_pixel(px, v, a, l.alpha);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (((q ^ px) >> (8 * c)) & 255u) p[c] = (uint8_t)(q >> (8 * c));
}

// The kernels: one calibration set for the launch (the tables in `l`), or -- _cal -- frame blockIdx.z with the tables of its own set.
// A pixel outside its own set's lane rows has lane value 0 (all four taps miss the bird's-eye image), so the union rows serve all.
__device__ __forceinline__ InplaceLane lane_of_slot(InplaceLane l, const OvTables* __restrict__ sets, const CalIds& ids) {
    const OvTables& o = SlotOv{sets, &ids}.of((int)blockIdx.z);
    l.oxy = o.oxy;
    l.ofrac = o.ofrac;
    return l;
}
__global__ __launch_bounds__(256) void k_inplace_rgb(const SurfEntry* __restrict__ tab, InplaceRows rows, InplaceLane l, InplaceText t,
                                                    int w, int items) {
    inplace_rgb_body(tab, rows, l, t, w, items);
}
__global__ __launch_bounds__(256) void k_inplace_rgb_cal(const SurfEntry* __restrict__ tab, InplaceRows rows, InplaceLane l, InplaceText t,
                                                        int w, int items, const OvTables* __restrict__ sets, CalIds ids) {
    inplace_rgb_body(tab, rows, lane_of_slot(l, sets, ids), t, w, items);
}

// byte layout of a quad's three dwords: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
__device__ __forceinline__ void inplace_rgb4_body(const SurfEntry* __restrict__ tab, const InplaceRows& rows, const InplaceLane& l,
                                                  const InplaceText& t, int w, int items) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= items) return;
    const int qrow = w >> 2, ri = i / qrow, xq = i - ri * qrow, y = row_of(rows, ri), z = (int)blockIdx.z;
    const int o = y * w + 4 * xq;
    const uint4 xy = reinterpret_cast<const uint4*>(l.oxy)[o >> 2];
    const uint2 fr = reinterpret_cast<const uint2*>(l.ofrac)[o >> 2];
    const uint32_t xyv[4] = {xy.x, xy.y, xy.z, xy.w};
    const uint32_t frv[4] = {fr.x & 0xffffu, fr.x >> 16, fr.y & 0xffffu, fr.y >> 16};
    const short2* sp = reinterpret_cast<const short2*>(l.spans) + (size_t)z * l.span_stride_rows;
    int v[4], a[4], any = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = lane_value(sp, l.bh, l.bw, (int16_t)(xyv[k] & 0xffffu), (int16_t)(xyv[k] >> 16), (int)frv[k]);
        a[k] = text_alpha(t, z, 4 * xq + k, y);
        any |= v[k] | a[k];
    }
    if (!any) return;
    const SurfEntry& e = tab[z];
    uint32_t* p = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(e.plane[0]) + (size_t)y * e.pitch) + 3 * xq;
    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
    const uint32_t q0 = ia::draw_pixel(d0 & 0xffffffu, v[0], a[0], l.alpha);
    const uint32_t q1 = ia::draw_pixel((d0 >> 24) | ((d1 & 0xffffu) << 8), v[1], a[1], l.alpha);
    const uint32_t q2 = ia::draw_pixel((d1 >> 16) | ((d2 & 0xffu) << 16), v[2], a[2], l.alpha);
    const uint32_t q3 = ia::draw_pixel(d2 >> 8, v[3], a[3], l.alpha);
    const uint32_t n0 = q0 | (q1 << 24), n1 = (q1 >> 8) | (q2 << 16), n2 = (q2 >> 16) | (q3 << 8);
    if (n0 != d0) p[0] = n0;
    if (n1 != d1) p[1] = n1;
    if (n2 != d2) p[2] = n2;
}

__global__ __launch_bounds__(256) void k_inplace_rgb4(const SurfEntry* __restrict__ tab, InplaceRows rows, InplaceLane l, InplaceText t,
                                                     int w, int items) {
    inplace_rgb4_body(tab, rows, l, t, w, items);
}
__global__ __launch_bounds__(256) void k_inplace_rgb4_cal(const SurfEntry* __restrict__ tab, InplaceRows rows, InplaceLane l, InplaceText t,
                                                         int w, int items, const OvTables* __restrict__ sets, CalIds ids) {
    inplace_rgb4_body(tab, rows, lane_of_slot(l, sets, ids), t, w, items);
}

// LAYOUT 1: NV12 (rows of U, V pairs), 2: I420 (a U and a V plane).  `rows` are runs of CHROMA rows: a thread owns whole blocks.
template <int LAYOUT, bool WIDE>
__device__ __forceinline__ void inplace_420_body(const SurfEntry* __restrict__ tab, const InplaceRows& rows, const InplaceLane& l,
                                                 const InplaceText& t, const YuvCoef& kin, const sa::Rgb2Yuv& kout, int w, int groups, int items) {
    constexpr int NB = WIDE ? 4 : 1;                 // blocks per thread, side by side
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= items) return;
    const int ci = i / groups, xg = i - ci * groups, cr = row_of(rows, ci), x0 = xg * 2 * NB, z = (int)blockIdx.z;
    const short2* sp = reinterpret_cast<const short2*>(l.spans) + (size_t)z * l.span_stride_rows;
    int v[NB][4], a[NB][4], hit[NB], any = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        hit[j] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + 2 * j + (k & 1), y = 2 * cr + (k >> 1);
            v[j][k] = lane_at(l, sp, y * w + x);
            a[j][k] = text_alpha(t, z, x, y);
            hit[j] |= v[j][k] | a[j][k];
        }
        any |= hit[j];
    }
    if (!any) return;
    const SurfEntry& e = tab[z];
    uint8_t* py0 = reinterpret_cast<uint8_t*>(e.plane[0]) + (size_t)(2 * cr) * e.pitch + x0;
    uint8_t* py1 = py0 + e.pitch;
    uint8_t* pu = reinterpret_cast<uint8_t*>(e.plane[1]) + (size_t)cr * e.cpitch + (LAYOUT == 1 ? x0 : (x0 >> 1));
    uint8_t* pv = LAYOUT == 1 ? pu + 1 : reinterpret_cast<uint8_t*>(e.plane[2]) + (size_t)cr * e.cpitch + (x0 >> 1);
    uint32_t Y0[2 * NB], Y1[2 * NB], U[NB], V[NB];
    if constexpr (WIDE) {
        const uint2 r0 = *reinterpret_cast<const uint2*>(py0), r1 = *reinterpret_cast<const uint2*>(py1);
        const uint32_t w0[2] = {r0.x, r0.y}, w1[2] = {r1.x, r1.y};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            Y0[k] = (w0[k >> 2] >> (8 * (k & 3))) & 255u;
            Y1[k] = (w1[k >> 2] >> (8 * (k & 3))) & 255u;
        }
        if constexpr (LAYOUT == 1) {
            const uint2 c = *reinterpret_cast<const uint2*>(pu);
            const uint32_t cw[2] = {c.x, c.y};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                U[j] = (cw[j >> 1] >> (16 * (j & 1))) & 255u;
                V[j] = (cw[j >> 1] >> (16 * (j & 1) + 8)) & 255u;
            }
        } else {
            const uint32_t uw = *reinterpret_cast<const uint32_t*>(pu), vw = *reinterpret_cast<const uint32_t*>(pv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                U[j] = (uw >> (8 * j)) & 255u;
                V[j] = (vw >> (8 * j)) & 255u;
            }
        }
    } else {
        Y0[0] = py0[0], Y0[1] = py0[1], Y1[0] = py1[0], Y1[1] = py1[1];
        U[0] = pu[0], V[0] = pv[0];
    }
    unsigned ch[NB], all = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        ch[j] = 0;
        if (hit[j]) {
            ia::Block b{{Y0[2 * j], Y0[2 * j + 1], Y1[2 * j], Y1[2 * j + 1]}, U[j], V[j]};
            ch[j] = ia::draw_block(b, v[j], a[j], l.alpha, kin, kout);
            Y0[2 * j] = b.y[0], Y0[2 * j + 1] = b.y[1], Y1[2 * j] = b.y[2], Y1[2 * j + 1] = b.y[3];
            U[j] = b.u, V[j] = b.v;
        }
        all |= ch[j];
    }
    if (!all) return;
    if constexpr (WIDE) {
        // the 8 bytes of a row, or of the chroma pairs, go back as they came -- one store -- when one of them changed
        if (all & 3u) {
            uint32_t o[2] = {0u, 0u};
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k >> 2] |= Y0[k] << (8 * (k & 3));
            *reinterpret_cast<uint2*>(py0) = make_uint2(o[0], o[1]);
        }
        if (all & 12u) {
            uint32_t o[2] = {0u, 0u};
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k >> 2] |= Y1[k] << (8 * (k & 3));
            *reinterpret_cast<uint2*>(py1) = make_uint2(o[0], o[1]);
        }
        if (all & 16u) {
            if constexpr (LAYOUT == 1) {
                uint32_t o[2] = {0u, 0u};
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j >> 1] |= (U[j] | (V[j] << 8)) << (16 * (j & 1));
                *reinterpret_cast<uint2*>(pu) = make_uint2(o[0], o[1]);
            } else {
                *reinterpret_cast<uint32_t*>(pu) = U[0] | (U[1] << 8) | (U[2] << 16) | (U[3] << 24);
                *reinterpret_cast<uint32_t*>(pv) = V[0] | (V[1] << 8) | (V[2] << 16) | (V[3] << 24);
            }
        }
    } else {
        if (all & 1u) py0[0] = (uint8_t)Y0[0];
        if (all & 2u) py0[1] = (uint8_t)Y0[1];
        if (all & 4u) py1[0] = (uint8_t)Y1[0];
        if (all & 8u) py1[1] = (uint8_t)Y1[1];
        if (all & 16u) {
            pu[0] = (uint8_t)U[0];
            pv[0] = (uint8_t)V[0];
        }
    }
}

template <int LAYOUT, bool WIDE>
__global__ __launch_bounds__(256) void k_inplace_420(const SurfEntry* __restrict__ tab, InplaceRows rows, InplaceLane l, InplaceText t,
                                                    YuvCoef kin, sa::Rgb2Yuv kout, int w, int groups, int items) {
    inplace_420_body<LAYOUT, WIDE>(tab, rows, l, t, kin, kout, w, groups, items);
}
template <int LAYOUT, bool WIDE>
__global__ __launch_bounds__(256) void k_inplace_420_cal(const SurfEntry* __restrict__ tab, InplaceRows rows, InplaceLane l, InplaceText t,
                                                        YuvCoef kin, sa::Rgb2Yuv kout, int w, int groups, int items,
                                                        const OvTables* __restrict__ sets, CalIds ids) {
    inplace_420_body<LAYOUT, WIDE>(tab, rows, lane_of_slot(l, sets, ids), t, kin, kout, w, groups, items);
}

// two runs of rows -> disjoint, ordered runs (one where they meet); unit = 1: pixel rows, 2: chroma rows (a run covers every chroma
// row one of its pixel rows belongs to)
InplaceRows merge_runs(const int r[4], int unit, int h) {
    int a0 = std::max(r[0], 0) / unit, a1 = (std::min(r[1], h) + unit - 1) / unit;
    int b0 = std::max(r[2], 0) / unit, b1 = (std::min(r[3], h) + unit - 1) / unit;
    if (a1 <= a0) { a0 = b0; a1 = b1; b0 = b1 = 0; }
    if (b1 <= b0) return InplaceRows{a0, std::max(a1 - a0, 0), 0, 0};
    if (b0 < a0) { std::swap(a0, b0); std::swap(a1, b1); }
    if (b0 <= a1) return InplaceRows{a0, std::max(a1, b1) - a0, 0, 0};
    return InplaceRows{a0, a1 - a0, b0, b1 - b0};
}

}  // namespace

// slots of one launch: entries[0, n) are the host's mirror of tab[0, n) (device), read here for the launch's alignment only
int launch_inplace(hipStream_t s, int layout, const SurfEntry* tab, const SurfEntry* entries, int n, int h, int w, const int rows4[4],
                   InplaceLane l, InplaceText t, YuvCoef kin, const int32_t* rgb2yuv, OvSets per_slot) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    const bool cal = per_slot.sets != nullptr;
    const int Z = cal ? (int)CalIds::N : 32768;
    int launches = 0;
    for (int at = 0; at < n; at += Z) {
        const int m = std::min(n - at, Z);
        size_t ybits = 0, cbits = 0;
        for (int j = at; j < at + m; ++j) {
            ybits |= (size_t)entries[j].plane[0] | (size_t)entries[j].pitch;
            if (layout != 0) cbits |= (size_t)entries[j].plane[1] | (size_t)entries[j].cpitch;
            if (layout == 2) cbits |= (size_t)entries[j].plane[2];
        }
        const InplaceDraw d = advanced(l, t, at);
        const CalIds ids = cal ? pack_cal_ids(per_slot.ids + at, m) : CalIds{};
        if (layout == 0) {
            const InplaceRows rows = merge_runs(rows4, 1, h);
            const int nrows = rows.an + rows.bn;
            if (nrows <= 0) continue;
            const bool four = (w & 3) == 0 && (ybits & 3) == 0;
            const int items = four ? nrows * (w >> 2) : nrows * w;
            const dim3 grid((unsigned)((items + 255) / 256), 1, (unsigned)m);
            if (cal) hipLaunchKernelGGL(four ? k_inplace_rgb4_cal : k_inplace_rgb_cal, grid, dim3(256), 0, s, tab + at, rows, d.l, d.t, w, items, per_slot.sets, ids);
            else hipLaunchKernelGGL(four ? k_inplace_rgb4 : k_inplace_rgb, grid, dim3(256), 0, s, tab + at, rows, d.l, d.t, w, items);
            ++launches;
            continue;
        }
        const InplaceRows rows = merge_runs(rows4, 2, h);
        const int nrows = rows.an + rows.bn;
        if (nrows <= 0) continue;
        const sa::Rgb2Yuv kout = sa::coef_of(rgb2yuv);
        const bool wide = (w & 7) == 0 && (ybits & 7) == 0 && (cbits & (layout == 1 ? 7 : 3)) == 0;
        const int groups = wide ? w / 8 : w / 2, items = nrows * groups;
        const dim3 grid((unsigned)((items + 255) / 256), 1, (unsigned)m);
        if (cal) {
            auto k = layout == 1 ? (wide ? k_inplace_420_cal<1, true> : k_inplace_420_cal<1, false>) : (wide ? k_inplace_420_cal<2, true> : k_inplace_420_cal<2, false>);
            hipLaunchKernelGGL(k, grid, dim3(256), 0, s, tab + at, rows, d.l, d.t, kin, kout, w, groups, items, per_slot.sets, ids);
        } else {
            auto k = layout == 1 ? (wide ? k_inplace_420<1, true> : k_inplace_420<1, false>) : (wide ? k_inplace_420<2, true> : k_inplace_420<2, false>);
            hipLaunchKernelGGL(k, grid, dim3(256), 0, s, tab + at, rows, d.l, d.t, kin, kout, w, groups, items);
        }
        ++launches;
    }
    return launches;
}

}  // namespace lt
