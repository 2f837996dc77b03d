// Input frames of another size than the calibration's (lt_set_input_size): cv2.resize(frame, img_size), INTER_LINEAR, of a run of
// destination rows, from the slots' staging frames (RGB, 3 B/px, the input's size) into the slots' RGB camera frames.
//   k_resize_rows<WIDE>   grid (groups of 64 x 4 destination columns, destination rows [a, b), slots)
// A thread owns four consecutive pixels of one destination row.  The two horizontal taps of a pixel are adjacent pixels of a tap
// row (or one pixel twice, the second with coefficient 0): 6 consecutive bytes, fetched as ONE 8-byte window per tap row -- the three
// aligned dwords that hold it through a buffer resource that covers the slot's staging frame, shifted into place with
// v_alignbyte_b32, as the RGB undistortion fetches its taps (k_frontend.hip) -- instead of twelve byte loads.  A window that ends
// behind the frame's last byte comes back as zeros from the resource's range check beyond the dword that holds that byte, and what
// a window holds beyond the two taps is never used; the context pads every staging frame so that this dword is its own.  The
// arithmetic is resize_arith.h's: 24-bit multiplies only.
//   WIDE: the destination width is a multiple of 4 and frame base and stride are dword-aligned -- every thread has its four pixels
//   and stores them as three dwords.  Otherwise the same walk stores byte by byte and masks the columns behind the row.
// Rows outside [a, b) are neither read nor written; the vertical taps of a row are block-uniform and arrive by scalar loads.
#include "lt_internal.h"
#include "resize_arith.h"

namespace lt {
namespace {

constexpr int RSRC_RAW = 0x00027000;   // untyped 32-bit buffer, no swizzle
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));

// the pixels (R | G << 8 | B << 16 in the low 24 bits; the top byte is whatever follows) at the two taps of the window of tap row
// `row_off` (bytes from the frame's start) of destination column entry `cw`
__device__ __forceinline__ void taps_of_row(__amdgpu_buffer_rsrc_t rs, uint32_t row_off, uint32_t cw, uint32_t& p0, uint32_t& p1) {
    const uint32_t off = row_off + (cw & 0xffffu);
    const u32x3 d = __builtin_amdgcn_raw_buffer_load_b96(rs, (int)(off & ~3u), 0, 0);
    const uint32_t lo = __builtin_amdgcn_alignbyte(d.y, d.x, off & 3u), hi = __builtin_amdgcn_alignbyte(d.z, d.y, off & 3u);
    p0 = __builtin_amdgcn_alignbyte(hi, lo, ((cw >> 16) & 1u) * 3u);
    p1 = __builtin_amdgcn_alignbyte(hi, lo, ((cw >> 17) & 1u) * 3u);
}

// xt: two words per destination column (rz::pack_column), padded to a multiple of four columns; yt: (tap0, tap1, c0, c1) per
// destination row.  src: staging frame of the launch's first slot, src_stride apart, src_bytes each; dst likewise.
template <bool WIDE>
__global__ __launch_bounds__(64) void k_resize_rows(const uint8_t* __restrict__ src, size_t src_stride, uint32_t src_bytes, int src_row_bytes,
                                                    uint8_t* __restrict__ dst, size_t dst_stride, int w, int row0,
                                                    const uint4* __restrict__ xt, const int4* __restrict__ yt) {
    const int x0 = 4 * (int)(blockIdx.x * 64 + threadIdx.x);
    if (x0 >= w) return;
    const int y = row0 + (int)blockIdx.y;
    const int4 ty = yt[y];
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(src) + (size_t)blockIdx.z * src_stride, 0,
                                                                        (int)((src_bytes + 3u) & ~3u), RSRC_RAW);
    const uint32_t r0 = (uint32_t)__mul24(ty.x, src_row_bytes), r1 = (uint32_t)__mul24(ty.y, src_row_bytes);
    const uint32_t b0 = (uint32_t)ty.z, b1 = (uint32_t)ty.w;
    const uint4 ca = xt[x0 >> 1], cb = xt[(x0 >> 1) + 1];
    const uint32_t cw[4] = {ca.x, ca.z, cb.x, cb.z}, cc[4] = {ca.y, ca.w, cb.y, cb.w};
    uint32_t px[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t p00, p01, p10, p11;
        taps_of_row(rs, r0, cw[j], p00, p01);
        taps_of_row(rs, r1, cw[j], p10, p11);
        const uint32_t a0 = cc[j] & 0xffffu, a1 = cc[j] >> 16;
        uint32_t v = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            v |= rz::resize_blend((p00 >> (8 * ch)) & 255u, (p01 >> (8 * ch)) & 255u, (p10 >> (8 * ch)) & 255u, (p11 >> (8 * ch)) & 255u,
                                  a0, a1, b0, b1) << (8 * ch);
        px[j] = v;
    }
    uint8_t* o = dst + (size_t)blockIdx.z * dst_stride + ((size_t)y * w + x0) * 3;
    if constexpr (WIDE) {
        uint32_t* q = reinterpret_cast<uint32_t*>(o);
        q[0] = px[0] | (px[1] << 24);
        q[1] = (px[1] >> 8) | (px[2] << 16);
        q[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        const int npx = min(4, w - x0);
        for (int j = 0; j < npx; ++j) {
            o[3 * j] = (uint8_t)px[j];
            o[3 * j + 1] = (uint8_t)(px[j] >> 8);
            o[3 * j + 2] = (uint8_t)(px[j] >> 16);
        }
    }
}

}  // namespace

void launch_resize_rows(hipStream_t s, const uint8_t* src, size_t src_stride, size_t src_bytes, int src_w, uint8_t* dst, size_t dst_stride,
                        int w, int a, int b, const uint32_t* xt, const int32_t* yt, int n) {
    if (n <= 0 || b <= a || w <= 0) return;
    const dim3 grid((unsigned)(((w + 3) / 4 + 63) / 64), (unsigned)(b - a), (unsigned)n);
    const bool wide = (w & 3) == 0 && (((uintptr_t)dst | dst_stride) & 3) == 0;
    if (wide)
        hipLaunchKernelGGL(k_resize_rows<true>, grid, dim3(64), 0, s, src, src_stride, (uint32_t)src_bytes, src_w * 3, dst, dst_stride, w, a,
                           reinterpret_cast<const uint4*>(xt), reinterpret_cast<const int4*>(yt));
    else
        hipLaunchKernelGGL(k_resize_rows<false>, grid, dim3(64), 0, s, src, src_stride, (uint32_t)src_bytes, src_w * 3, dst, dst_stride, w, a,
                           reinterpret_cast<const uint4*>(xt), reinterpret_cast<const int4*>(yt));
}

}  // namespace lt
