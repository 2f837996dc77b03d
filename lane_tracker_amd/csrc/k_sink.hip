// Device sinks: dense RGB frames of the library (the annotated frames of a context, d_annot) -> surfaces the caller owns, in the
// caller's pixel format and pitches -- RGB (a pitched row copy), BGR / RGBA / BGRA (the same copy with permuted channels, alpha
// written as 255), NV12 or I420 (sink_arith.h: OpenCV's RGB2YUV_I420 arithmetic,
// chroma from the pixel at the even row and even column of each 2 x 2 block).  The mirror image of k_rows_to_rgb /
// k_surf_copy_rows (k_frontend.hip).  The destinations of a launch travel as a SurfChunk kernel argument (frame blockIdx.z is
// entry blockIdx.z).
//
// Every store lands inside a row's own bytes of its own plane: 16 (8) bytes at a column that is a multiple of 16 (8) in a row
// whose length is one too, or single bytes.  Nothing is written between rows or around planes -- those bytes are the caller's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "lt_internal.h"
#include "sink_arith.h"

namespace lt {

using sa::Rgb2Yuv;

// One thread owns the two rows of chroma row cr over the 16 columns from x0: 48 source bytes per row in three 16-byte loads, 16 Y
// bytes per row in one 16-byte store, and the 8 (U, V) of the even-row, even-column pixels -- NV12: one 16-byte store of pairs,
// I420: 8 bytes each.  Threads are numbered along the rows of chroma rows (`groups` = w / 16 threads each), so a wave's loads
// cover 3 KB of consecutive source bytes and its Y stores 1 KB of a row.
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_rgb_rows_to_surf(const uint8_t* __restrict__ rgb, size_t rgb_stride, SurfChunk ch, Rgb2Yuv k,
                                                         int w, int groups, int items) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t >= items) return;
    const int cr = t / groups, x0 = (t - cr * groups) * 16;
    const SurfEntry& e = ch.e[blockIdx.z];
    const uint8_t* src = rgb + (size_t)blockIdx.z * rgb_stride;
    uint32_t cu[2] = {0u, 0u}, cv[2] = {0u, 0u};           // 8 U, 8 V
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * cr + dy;
        const uint4* s = reinterpret_cast<const uint4*>(src + ((size_t)y * w + x0) * 3);
        const uint4 q0 = s[0], q1 = s[1], q2 = s[2];
        const uint32_t d[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        uint32_t yo[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = (int)((d[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255u);
            const int g = (int)((d[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255u);
            const int b = (int)((d[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255u);
            yo[i >> 2] |= sa::luma(r, g, b, k) << (8 * (i & 3));
            if (dy == 0 && (i & 1) == 0) {
                cu[i >> 3] |= sa::chroma_u(r, g, b, k) << (8 * ((i >> 1) & 3));
                cv[i >> 3] |= sa::chroma_v(r, g, b, k) << (8 * ((i >> 1) & 3));
            }
        }
        *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(e.plane[0]) + (size_t)y * e.pitch + x0) = make_uint4(yo[0], yo[1], yo[2], yo[3]);
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
    } else {
        const size_t co = (size_t)cr * e.cpitch + (size_t)(x0 >> 1);
        *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(e.plane[1]) + co) = make_uint2(cu[0], cu[1]);
        *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(e.plane[2]) + co) = make_uint2(cv[0], cv[1]);
    }
}

// the same for any even width, any pitch and any alignment: one thread per 2 x 2 block (`groups` = w / 2 of them per chroma
// row), byte accesses
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_rgb_rows_to_surf_any(const uint8_t* __restrict__ rgb, size_t rgb_stride, SurfChunk ch, Rgb2Yuv k,
                                                             int w, int groups, int items) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t >= items) return;
    const int cr = t / groups, bx = t - cr * groups;
    const SurfEntry& e = ch.e[blockIdx.z];
    const uint8_t* src = rgb + (size_t)blockIdx.z * rgb_stride;
    uint8_t* py = reinterpret_cast<uint8_t*>(e.plane[0]);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * cr + dy;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const uint8_t* px = src + ((size_t)y * w + 2 * bx + dx) * 3;
            const int r = px[0], g = px[1], b = px[2];
            py[(size_t)y * e.pitch + 2 * bx + dx] = (uint8_t)sa::luma(r, g, b, k);
            if (dy == 0 && dx == 0) {
                const uint8_t u = (uint8_t)sa::chroma_u(r, g, b, k), v = (uint8_t)sa::chroma_v(r, g, b, k);
                const size_t crow = (size_t)cr * e.cpitch;
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

// The RGB sink: the rows of dense RGB frames (row_bytes = 3 w) -> the same rows of RGB surfaces, a pitched row copy -- one thread
// per 16 bytes (WIDE: row_bytes and every base and pitch of the launch a multiple of 16) or per byte.  k_surf_copy_rows, reversed.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_rgb_copy_rows_to_surf(const uint8_t* __restrict__ rgb, size_t rgb_stride, SurfChunk ch, int row_bytes) {
    constexpr int V = WIDE ? 16 : 1;
    const int xb = (int)(blockIdx.x * 256u + threadIdx.x) * V;
    if (xb >= row_bytes) return;
    const int y = (int)blockIdx.y;
    const SurfEntry& e = ch.e[blockIdx.z];
    const uint8_t* src = rgb + (size_t)blockIdx.z * rgb_stride + (size_t)y * row_bytes + xb;
    uint8_t* dst = reinterpret_cast<uint8_t*>(e.plane[0]) + (size_t)y * e.pitch + xb;
    if constexpr (WIDE) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    else *dst = *src;
}

// The RGB family's other members (F = the layout: 5 BGR, 6 RGBA, 7 BGRA): the pitched copy above with the channels permuted and,
// for the 4-byte pixels, alpha = 255.  WIDE (w a multiple of 16, every base and pitch of the launch one too): one thread per 16
// pixels, 48 bytes in three 16-byte loads, 48 / 64 bytes in three / four 16-byte stores; else one thread per pixel, byte stores.
template <int F, bool WIDE>
__global__ __launch_bounds__(256) void k_rgb_rows_to_px(const uint8_t* __restrict__ rgb, size_t rgb_stride, SurfChunk ch, int w) {
    constexpr int BPP = F == 5 ? 3 : 4, R = F == 6 ? 0 : 2, B = 2 - R;
    const int x = (int)(blockIdx.x * 256u + threadIdx.x) * (WIDE ? 16 : 1);
    if (x >= w) return;
    const int y = (int)blockIdx.y;
    const SurfEntry& e = ch.e[blockIdx.z];
    const uint8_t* src = rgb + (size_t)blockIdx.z * rgb_stride + ((size_t)y * w + x) * 3;
    uint8_t* dst = reinterpret_cast<uint8_t*>(e.plane[0]) + (size_t)y * e.pitch + (size_t)x * BPP;
    if constexpr (WIDE) {
        const uint4* s = reinterpret_cast<const uint4*>(src);
        const uint4 q0 = s[0], q1 = s[1], q2 = s[2];
        const uint32_t d[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        uint32_t o[4 * BPP] = {};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t c[3] = {(d[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255u, (d[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255u,
                                   (d[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255u};
            const int b0 = BPP * i;
            o[(b0 + R) >> 2] |= c[0] << (8 * ((b0 + R) & 3));
            o[(b0 + 1) >> 2] |= c[1] << (8 * ((b0 + 1) & 3));
            o[(b0 + B) >> 2] |= c[2] << (8 * ((b0 + B) & 3));
            if constexpr (BPP == 4) o[i] |= 255u << 24;
        }
        uint4* out = reinterpret_cast<uint4*>(dst);
#pragma unroll
        for (int i = 0; i < BPP; ++i) out[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
    } else {
        dst[R] = src[0];
        dst[1] = src[1];
        dst[B] = src[2];
        if constexpr (BPP == 4) dst[3] = 255;
    }
}

template <int F>
static void launch_rgb_rows_to_px(hipStream_t s, bool wide, const uint8_t* src, size_t rgb_stride, const SurfChunk& ch, int h, int w, int m) {
    if (wide)
        hipLaunchKernelGGL((k_rgb_rows_to_px<F, true>), dim3((unsigned)((w / 16 + 255) / 256), (unsigned)h, (unsigned)m), dim3(256), 0, s, src, rgb_stride, ch, w);
    else
        hipLaunchKernelGGL((k_rgb_rows_to_px<F, false>), dim3((unsigned)((w + 255) / 256), (unsigned)h, (unsigned)m), dim3(256), 0, s, src, rgb_stride, ch, w);
}

// n frames -> entries[0, n) (host memory, consumed before the call returns); the wide kernels where a launch's geometry allows them
void launch_rgb_to_surfaces(hipStream_t s, int layout, const uint8_t* rgb, size_t rgb_stride, int h, int w, const SurfEntry* entries,
                            int n, const int32_t* coeffs) {
    if (n <= 0 || h <= 0 || w <= 0) return;
    const Rgb2Yuv k = layout == 1 || layout == 2 ? sa::coef_of(coeffs) : Rgb2Yuv{};
    for (int i = 0; i < n; i += SurfChunk::N) {
        const int m = std::min(n - i, (int)SurfChunk::N);
        SurfChunk ch{};
        std::copy(entries + i, entries + i + m, ch.e);
        const uint8_t* src = rgb + (size_t)i * rgb_stride;
        size_t bits = rgb_stride | (size_t)(uintptr_t)src, cbits = 0;   // every base and pitch of the launch a multiple of 16 (I420 chroma: 8)?
        for (int j = 0; j < m; ++j) {
            bits |= (size_t)ch.e[j].plane[0] | (size_t)ch.e[j].pitch;
            if (layout == 1) bits |= (size_t)ch.e[j].plane[1] | (size_t)ch.e[j].cpitch;
            if (layout == 2) cbits |= (size_t)ch.e[j].plane[1] | (size_t)ch.e[j].plane[2] | (size_t)ch.e[j].cpitch;
        }
        if (layout == 0) {
            const int row_bytes = w * 3;
            if ((bits & 15) == 0 && (row_bytes & 15) == 0)
                hipLaunchKernelGGL(k_rgb_copy_rows_to_surf<true>, dim3((unsigned)((row_bytes / 16 + 255) / 256), (unsigned)h, (unsigned)m), dim3(256), 0, s, src, rgb_stride, ch, row_bytes);
            else
                hipLaunchKernelGGL(k_rgb_copy_rows_to_surf<false>, dim3((unsigned)((row_bytes + 255) / 256), (unsigned)h, (unsigned)m), dim3(256), 0, s, src, rgb_stride, ch, row_bytes);
        } else if (layout >= 5) {
            const bool wide = (w & 15) == 0 && (bits & 15) == 0;
            if (layout == 5) launch_rgb_rows_to_px<5>(s, wide, src, rgb_stride, ch, h, w, m);
            else if (layout == 6) launch_rgb_rows_to_px<6>(s, wide, src, rgb_stride, ch, h, w, m);
            else launch_rgb_rows_to_px<7>(s, wide, src, rgb_stride, ch, h, w, m);
        } else if ((w & 15) == 0 && (bits & 15) == 0 && (cbits & 7) == 0) {
            const int groups = w / 16, items = (h / 2) * groups;
            hipLaunchKernelGGL(layout == 1 ? k_rgb_rows_to_surf<1> : k_rgb_rows_to_surf<2>, dim3((unsigned)((items + 255) / 256), 1, (unsigned)m), dim3(256), 0, s,
                               src, rgb_stride, ch, k, w, groups, items);
        } else {
            const int groups = w / 2, items = (h / 2) * groups;
            hipLaunchKernelGGL(layout == 1 ? k_rgb_rows_to_surf_any<1> : k_rgb_rows_to_surf_any<2>, dim3((unsigned)((items + 255) / 256), 1, (unsigned)m), dim3(256), 0, s,
                               src, rgb_stride, ch, k, w, groups, items);
        }
    }
}

}  // namespace lt
