// Geometric front end + colour split, gfx950.
//
//   k_undistort_rows<LAYOUT, SRC, PER_SLOT>  cv2.undistort  lane_tracker.py:832   (only the rows the warp reads): the one entry point of
//                      the one walk, undistort_walk<source, pixel format>.  LAYOUT, the frames' pixel format: 0 RGB; 1 NV12, 2 I420
//                      (cv2.cvtColor(YUV2RGB_*) of every tap, then the blend); 3 YUY2, 4 UYVY (packed 4:2:2); 5 BGR, 6 RGBA, 7 BGRA (a
//                      channel permutation, folded into the shifts the walk takes its channels out with); 16 .. 19 8-bit raw Bayer RGGB /
//                      GRBG / GBRG / BGGR (every tap demosaiced -- bilinear, bayer_arith.h -- from one 4 x 4 byte window).  SRC: 0 frames
//                      in the caller's device memory (surface table), 1 / 2 the slots' own frames, dword-aligned / at any byte (RGB).
//                      PER_SLOT: every slot of a launch with the remap tables of its own calibration set (lt_add_calibration), for
//                      slices that mix sets; k_warp_cal: the same form of the warp
//   k_rows_to_rgb<LAYOUT, SURF, WIDE>  a run of rows of frames in LAYOUT (not 0) as RGB, for whoever shows the camera frame
//                      (cv2.cvtColor(YUV2RGB_NV12 / _I420 / _YUY2 / _UYVY), a permutation, the demosaic), from a slot's staging frame / from
//                      a surface (SURF): one 16-column (WIDE) and one byte-wise body per family of layouts; k_surf_copy_rows: RGB surfaces
//   k_raw_walk_rows<PATTERN, SRC, PER_SLOT, STAGES>, k_raw_rows_rgb<PATTERN, SURF, WIDE, STAGES>  the two above for raw Bayer frames behind
//                      a raw table staged in LDS, launched in their place whenever there is one; what else runs around the demosaic is
//                      STAGES, and its operands one RawStages (lt_internal.h).  Bit 0: 10- / 12-bit frames (layouts 32 .. 35, 48 .. 51:
//                      16-bit little-endian words, the sample in the low `bits` bits, a run-time argument) behind their wide table
//                      (lt_set_raw_lut_wide: 1 << bits entries per colour phase, 4 KB / 16 KB of dynamic LDS), every site masked and looked
//                      up into the 8-bit window that the 8-bit demosaic takes; else 8-bit frames behind lt_set_raw_lut's table (black level,
//                      white balance and tone curve as 256 entries per colour phase), every byte looked up before it is demosaiced.  Bit 1:
//                      the colour stage (lt_set_raw_color) on every demosaiced tap / pixel -- a colour-correction matrix (Q10, nine scalar
//                      operands of 24-bit multiply-adds), a clamp and a 256-entry output curve staged in LDS with the table.  Bit 2: the
//                      lens-shading correction (lt_set_raw_shading; shade_arith.h), every sample corrected by the gain of its site before
//                      its table lookup; the gains lie in a plane that k_shade_expand makes of the map's mesh once, and a walk loads the
//                      16 of its window once and keeps them across its frames
//   k_mipi_walk_rows<PATTERN, SRC, PER_SLOT, STAGES, PACK>, k_mipi_rows_rgb<PATTERN, SURF, WIDE, STAGES, PACK>  the two above over MIPI-packed
//                      RAW10 / RAW12 frames (layouts 36 .. 39, 52 .. 55: one plane of bytes, PACK 0 five bytes for four sites, 1 three bytes
//                      for two; mipi_arith.h), STAGES 1, 3, 5, 7: the 16-bit forms with every window row (every site, every 16 columns of
//                      the row conversion) unpacked into 16-bit words on its way in -- the same 96-bit window loads, table, LDS and
//                      staging; byte permutes and packed shifts with selectors found once per walk, no memory instruction added
//   k_rawset_walk_rows<PATTERN, SRC, STAGES>, k_packset_walk_rows<PATTERN, SRC, STAGES, PACK>, k_rawset_rows_rgb<PATTERN, SURF, WIDE, STAGES>,
//   k_packset_rows_rgb<.., PACK>  the four raw kernels above for a launch whose slots mix raw sets (lt_add_raw_set): a workgroup serves one
//                      slot and takes the operands the one-set kernels get as their RawStages from its slot's entry of the context's
//                      table of raw sets (raw_setup.h: RawSetEntry), by scalar loads; STAGES is the union of what the sets have.  The
//                      bodies are the one-set kernels', shared as device functions (raw_walk, mipi_walk, raw_rows)
//   k_warp_split       cv2.warpPerspective      lane_tracker.py:834
//                      + img[:,:,0]             lane_tracker.py:207
//                      + cvtColor(RGB2LAB)[:,:,2] lane_tracker.py:208
//
// Both resamplings are OpenCV's 8-bit bilinear remap: integer tap (sx,sy) + 5-bit fractions,
// exact 15-bit weights, constant-0 border, (sum + 2^14) >> 15.  They cannot be composed into one
// resampling because the intermediate is rounded to u8, so the undistorted rows are materialised
// once (one RGBX dword per pixel, rows x W x 4 bytes per frame: it stays in L2 for the warp).
// The bird's-eye RGB image itself is never written: the warp emits the R plane and the Lab-b
// plane directly.
//
// Layout of the undistorted rows: slots 2p and 2p+1 are INTERLEAVED per pixel (lt_internal.h: und_slot_base; pixel i
// of slot s is dword und_slot_base(s) + 2 i).  Both remap kernels are bound by the NUMBER of vector-memory
// instructions they issue (profiles/r02_vmem_issue.json: ~20 cycles of a CU's memory pipe per wave-instruction whatever
// its width), and with this layout the two horizontally adjacent taps of a bilinear sample are 16 contiguous bytes that
// hold them for two frames: one dwordx4 load instead of two dwordx2 loads.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "bayer_arith.h"
#include "front_arith.h"
#include "lt_internal.h"
#include "mipi_arith.h"
#include "shade_arith.h"
#include "yuv_arith.h"

namespace lt {
namespace {

// Every product in this file fits 24 bits, so the multiplies are written with __mul24: a plain 32-bit
// `*` becomes v_mul_lo_u32, which issues at a quarter of the v_mul_u32_u24 / v_mad_u32_u24 rate.
__device__ __forceinline__ int bilerp(int v00, int v01, int v10, int v11, int fx, int fy) {
    const int gx = 32 - fx, gy = 32 - fy;
    // (sum_i w_i v_i + 2^14) >> 15 with w = {gx gy, fx gy, gx fy, fx fy} * 32  ==  (gy h0 + fy h1 + 512) >> 10
    const int h0 = __mul24(v00, gx) + __mul24(v01, fx), h1 = __mul24(v10, gx) + __mul24(v11, fx);
    return (__mul24(h0, gy) + __mul24(h1, fy) + 512) >> 10;
}

// Workgroups are dealt to the 8 XCDs round-robin in linear launch order (x fastest, then y, then z), and each XCD
// has its own L2.  `xcd_block` turns the hardware's linear id into the id this workgroup works on, such that every
// XCD owns one contiguous range of the launch: neighbouring blocks sample overlapping source rows, and with the
// round-robin order each of the 8 L2s fetched its own copy of them (rocprofv3 FETCH_SIZE of the warp: 2.5x the
// source bytes).  Bijective for any launch size; speed only, never correctness.  remap == 0: identity.
__device__ __forceinline__ uint32_t xcd_block(uint32_t lid, uint32_t total, int remap) {
    if (!remap) return lid;
    const uint32_t q = total >> 3, r = total & 7u, xcd = lid & 7u, k = lid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// ---- YUV 4:2:0 input ------------------------------------------------------------------------------------------------------
// OpenCV's 8-bit YUV -> RGB, one (U, V) pair per 2 x 2 block, no chroma interpolation: yuv_arith.h (shared with k_inplace.hip and
// compiled for the host by the CPU tests).
using ya::Chroma;
using ya::yuv_chroma;
using ya::yuv_pixel;

// ---- the undistortion walk --------------------------------------------------------------------------------------------------
// One thread per undistorted pixel, walking the frames of its launch slice with one remap-table entry; the output is one RGBX
// dword per pixel, so that the warp fetches a whole tap with a single aligned load.  undistort_walk below is the only walk: a
// pixel FORMAT says which windows of bytes a sample needs (plane, row, byte column) and turns them into the four RGB taps, a
// SOURCE says where the planes of frame z lie and fetches a window.  Every window is fetched unconditionally from a clamped
// address and the taps are masked afterwards (a guarded load serialises on its own s_waitcnt).
constexpr int RSRC_RAW = 0x00027000;   // untyped 32-bit buffer, no swizzle
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));

// The sizeof(W) = 4 / 8 bytes at byte `off` (+ the scalar `soff`) of a buffer: the two / three aligned dwords that hold them,
// shifted into place with v_alignbyte_b32 -- an unaligned dwordx2 at 3-byte pitch occupies the memory pipe for ~32 cycles, an
// aligned dwordx3 for ~20.  What a window holds beyond the samples it was fetched for is never used.
// sizeof(W) = 12 (Bytes12): all that those three dwords hold from byte `off` on, the last 0 .. 3 bytes zero.
struct Bytes12 { uint32_t w0, w1, w2; };
template <class W>
__device__ __forceinline__ W window_at(__amdgpu_buffer_rsrc_t rs, uint32_t off, int soff) {
    if constexpr (sizeof(W) == 12) {
        const u32x3 d = __builtin_amdgcn_raw_buffer_load_b96(rs, (int)(off & ~3u), soff, 0);
        return W{__builtin_amdgcn_alignbyte(d.y, d.x, off & 3u), __builtin_amdgcn_alignbyte(d.z, d.y, off & 3u), __builtin_amdgcn_alignbyte(0u, d.z, off & 3u)};
    } else if constexpr (sizeof(W) == 8) {
        const u32x3 d = __builtin_amdgcn_raw_buffer_load_b96(rs, (int)(off & ~3u), soff, 0);
        const uint32_t lo = __builtin_amdgcn_alignbyte(d.y, d.x, off & 3u), hi = __builtin_amdgcn_alignbyte(d.z, d.y, off & 3u);
        return (uint64_t)lo | ((uint64_t)hi << 32);
    } else {
        const u32x2 d = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(off & ~3u), soff, 0);
        return __builtin_amdgcn_alignbyte(d.y, d.x, off & 3u);
    }
}

// A plane of a frame as its format defines it; `dense` = where it starts in a slot's own (unpitched) frame.
struct PlaneGeom { int rows, row_bytes; uint32_t dense; };
// The clamped columns of a sample's two taps: cx0, cx1 (both in {cxl, cxl + 1}) and the leftmost column cxl of what is fetched.
struct TapCols { int cxl, cx0, cx1; };

// RGB interleaved, 3 B/px.  The two taps of a row are 6 consecutive bytes (RGB RGB) at byte 3 * cxl: one 8-byte window per tap
// row instead of six byte loads.  When sx or sx + 1 is outside the frame the row is fetched from the clamped column and the
// taps are masked.  A format also says at which bit of a decoded tap channel ch (0: R, 1: G, 2: B) lies -- chan(ch), 8 * ch for
// R G B order; REVERSED: bytes B G R (OpenCV's BGR), chan(ch) = 16 - 8 * ch: another constant in the same shift, no instruction.
template <bool REVERSED>
struct Rgb24T {
    typedef uint64_t Window;
    static constexpr int DENSE_PAD = 8;     // a slot's frame buffer is padded by 8 bytes: the window of its last pixel ends there
    static constexpr int chan(int ch) { return REVERSED ? 16 - 8 * ch : 8 * ch; }
    struct Taps { uint64_t a, b; };          // the windows of the upper (a) and the lower (b) tap row
    int col, sh0, sh1;
    __device__ __forceinline__ void place(const TapCols& c) {
        col = c.cxl * 3;
        sh0 = 24 * (c.cx0 - c.cxl), sh1 = 24 * (c.cx1 - c.cxl);   // column cx sits at byte 3 * (cx - cxl) of the window
    }
    __device__ __forceinline__ static PlaneGeom plane(const FrontEndGeom& g, int) { return PlaneGeom{g.img_h, g.img_w * 3, 0u}; }
    template <class Source>
    __device__ __forceinline__ Taps fetch(const Source& src, const typename Source::Frame& f, const FrontEndGeom& g, int cy0, int cy1) const {
        const auto p0 = src.plane(f, plane(g, 0), 0);
        return Taps{src.template window<Window>(p0, cy0, col), src.template window<Window>(p0, cy1, col)};
    }
    __device__ __forceinline__ void decode(const Taps& t, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) const {
        a0 = (uint32_t)(t.a >> sh0), a1 = (uint32_t)(t.a >> sh1);
        b0 = (uint32_t)(t.b >> sh0), b1 = (uint32_t)(t.b >> sh1);
    }
};
typedef Rgb24T<false> Rgb24;
typedef Rgb24T<true> Bgr24;

// Four bytes a pixel, the fourth (alpha, or padding: RGBx / BGRx) never used.  ORDER 0: R G B A, 1: B G R A.  The two taps of a tap
// row are the two dwords at byte 4 * cxl (cxl <= W - 2: the window never leaves its row); a tap is the dword of its column, a select.
// From a slot's staging frame the window is dword-aligned: a plain two-dword fetch.
template <int ORDER>
struct Rgb32 {
    typedef uint64_t Window;
    static constexpr int DENSE_PAD = 8;
    static constexpr int chan(int ch) { return ORDER ? 16 - 8 * ch : 8 * ch; }
    struct Taps { uint64_t a, b; };
    int col, hi0, hi1;
    __device__ __forceinline__ void place(const TapCols& c) {
        col = c.cxl * 4;
        hi0 = c.cx0 - c.cxl, hi1 = c.cx1 - c.cxl;           // column cx is dword cx - cxl (0 / 1) of the window
    }
    __device__ __forceinline__ static PlaneGeom plane(const FrontEndGeom& g, int) { return PlaneGeom{g.img_h, g.img_w * 4, 0u}; }
    template <class Source>
    __device__ __forceinline__ Taps fetch(const Source& src, const typename Source::Frame& f, const FrontEndGeom& g, int cy0, int cy1) const {
        const auto p0 = src.plane(f, plane(g, 0), 0);
        return Taps{src.dwords2(p0, cy0, col), src.dwords2(p0, cy1, col)};
    }
    __device__ __forceinline__ static uint32_t pick(uint64_t w, int hi) { return hi ? (uint32_t)(w >> 32) : (uint32_t)w; }
    __device__ __forceinline__ void decode(const Taps& t, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) const {
        a0 = pick(t.a, hi0), a1 = pick(t.a, hi1);
        b0 = pick(t.b, hi0), b1 = pick(t.b, hi1);
    }
};
// the formats of layouts 5 (BGR), 6 (RGBA), 7 (BGRA)
template <int F> using PxFormat = std::conditional_t<F == 5, Bgr24, Rgb32<F == 7 ? 1 : 0>>;

// 4:2:0.  LAYOUT 1: NV12 (Y plane, then rows of U,V pairs), 2: I420 (Y, U, V planes).  Conversion is not linear (the clamps, the
// shift), so each of the four taps is converted before the blend.  Per tap row: the 4-byte window that holds the two Y samples
// and the 4-byte window(s) that hold the one or two chroma pairs under them -- 4 loads per frame for NV12, 6 for I420.
template <int LAYOUT>
struct Yuv420 {
    typedef uint32_t Window;
    static constexpr int DENSE_PAD = 16;    // a slot's staging frame: 16 bytes of padding behind the last slot
    static constexpr int chan(int ch) { return 8 * ch; }   // (yuv_pixel: R | G << 8 | B << 16)
    struct Taps { uint32_t ya, yb, ca, cb, va, vb; };      // Y and chroma windows of the upper (a) and lower (b) tap row; va / vb: I420's V
    YuvCoef k;
    int cxl, ccol, ysh0, ysh1, cs0, cs1;
    __device__ __forceinline__ void place(const TapCols& c) {
        cxl = c.cxl;                                       // (the width is even, so cxl >= 0)
        const int cb = c.cxl & ~1;                         // first column of the chroma pair under cxl; cxl + 1 is under cb or cb + 2
        ccol = LAYOUT == 1 ? cb : cb >> 1;                 // byte column of the chroma window in its plane
        ysh0 = 8 * (c.cx0 - c.cxl), ysh1 = 8 * (c.cx1 - c.cxl);                // the taps' Y samples inside the Y window
        cs0 = (c.cx0 - cb) >> 1, cs1 = (c.cx1 - cb) >> 1;                      // the taps' pair (0 / 1) inside the chroma window
    }
    __device__ __forceinline__ static PlaneGeom plane(const FrontEndGeom& g, int p) {
        const uint32_t luma = (uint32_t)__mul24(g.img_h, g.img_w);
        if (p == 0) return PlaneGeom{g.img_h, g.img_w, 0u};
        // I420's V plane lies (h / 2) (w / 2) bytes behind the U plane
        return PlaneGeom{g.img_h >> 1, LAYOUT == 1 ? g.img_w : g.img_w >> 1, p == 1 ? luma : luma + (luma >> 2)};
    }
    template <class Source>
    __device__ __forceinline__ Taps fetch(const Source& src, const typename Source::Frame& f, const FrontEndGeom& g, int cy0, int cy1) const {
        Taps t;
        const auto py = src.plane(f, plane(g, 0), 0), pc = src.plane(f, plane(g, 1), 1);
        t.ya = src.template window<Window>(py, cy0, cxl);
        t.yb = src.template window<Window>(py, cy1, cxl);
        t.ca = src.template window<Window>(pc, cy0 >> 1, ccol);
        t.cb = src.template window<Window>(pc, cy1 >> 1, ccol);
        if constexpr (LAYOUT == 2) {
            const auto pv = src.plane(f, plane(g, 2), 2);
            t.va = src.template window<Window>(pv, cy0 >> 1, ccol);
            t.vb = src.template window<Window>(pv, cy1 >> 1, ccol);
        } else {
            t.va = t.vb = 0;
        }
        return t;
    }
    __device__ __forceinline__ uint32_t tap(uint32_t yw, uint32_t cw, uint32_t vw, int ysh, int cs) const {
        int u, v;
        if constexpr (LAYOUT == 1) {
            u = (int)((cw >> (16 * cs)) & 255u);
            v = (int)((cw >> (16 * cs + 8)) & 255u);
        } else {
            u = (int)((cw >> (8 * cs)) & 255u);
            v = (int)((vw >> (8 * cs)) & 255u);
        }
        return yuv_pixel((int)((yw >> ysh) & 255u), yuv_chroma(u, v, k), k);
    }
    __device__ __forceinline__ void decode(const Taps& t, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) const {
        a0 = tap(t.ya, t.ca, t.va, ysh0, cs0), a1 = tap(t.ya, t.ca, t.va, ysh1, cs1);
        b0 = tap(t.yb, t.cb, t.vb, ysh0, cs0), b1 = tap(t.yb, t.cb, t.vb, ysh1, cs1);
    }
};

// Packed 4:2:2, one plane of 2 W bytes per row.  ORDER 0: YUY2 (Y0 U Y1 V), 1: UYVY (U Y0 V Y1).  The two taps of a tap row lie inside
// two consecutive macropixels: one 8-byte window per tap row, as for RGB -- 2 loads per frame.  The window starts at macropixel
// min(cxl >> 1, W / 2 - 2) (yuv_arith.h: the position arithmetic, which the CPU tests compile for the host), so it never leaves its
// row.  Each tap picks the dword of its macropixel (a select; no 64-bit shift) and is converted before the blend, as for 4:2:0; the
// two taps of a row may or may not share a macropixel, so both are converted.
template <int ORDER>
struct Yuv422 {
    typedef uint64_t Window;
    static constexpr int DENSE_PAD = 16;    // a slot's staging frame: 16 bytes of padding behind the last slot (the third dword of the last window's aligned load)
    static constexpr int chan(int ch) { return 8 * ch; }
    struct Taps { uint64_t a, b; };          // the windows of the upper (a) and the lower (b) tap row
    YuvCoef k;
    int last_mp;                             // W / 2 - 2
    int col, hi0, hi1, ysh0, ysh1;
    __device__ __forceinline__ void place(const TapCols& c) {
        const int mp = ya::win422_mp(c.cxl, last_mp);
        col = ya::win422_col(mp);
        hi0 = ya::win422_dword(c.cx0, mp), hi1 = ya::win422_dword(c.cx1, mp);
        ysh0 = ya::ysh422(ORDER, c.cx0), ysh1 = ya::ysh422(ORDER, c.cx1);
    }
    __device__ __forceinline__ static PlaneGeom plane(const FrontEndGeom& g, int) { return PlaneGeom{g.img_h, 2 * g.img_w, 0u}; }
    template <class Source>
    __device__ __forceinline__ Taps fetch(const Source& src, const typename Source::Frame& f, const FrontEndGeom& g, int cy0, int cy1) const {
        const auto p0 = src.plane(f, plane(g, 0), 0);
        return Taps{src.template window<Window>(p0, cy0, col), src.template window<Window>(p0, cy1, col)};
    }
    __device__ __forceinline__ uint32_t tap(uint64_t w, int hi, int ysh) const {
        return ya::yuv422_pixel(hi ? (uint32_t)(w >> 32) : (uint32_t)w, ORDER, ysh, k);
    }
    __device__ __forceinline__ void decode(const Taps& t, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) const {
        a0 = tap(t.a, hi0, ysh0), a1 = tap(t.a, hi1, ysh1);
        b0 = tap(t.b, hi0, ysh0), b1 = tap(t.b, hi1, ysh1);
    }
};

// 8-bit raw Bayer, one plane of W bytes per row.  PATTERN 0: RGGB, 1: GRBG, 2: GBRG, 3: BGGR (bayer_arith.h).  Demosaicing is not
// linear in the samples (the rounding shifts), so each of the four taps is demosaiced before the blend, at its position clamped to
// the interior.  The four 3 x 3 neighbourhoods lie inside one 4 x 4 byte window -- rows by .. by + 3 from byte column bx, by =
// clamp(sy - 1, 0, H - 4), bx = clamp(sx - 1, 0, W - 4) -- so a frame costs four 4-byte windows, as NV12 does, and no window leaves
// its row or the plane.  Each clamped tap sits at offset 1 or 2 inside the window in both directions; its colour phase follows from
// the parities of its clamped position and the pattern, a compile-time constant.
template <int PATTERN>
struct Bayer8 {
    typedef uint32_t Window;
    static constexpr int DENSE_PAD = 16;    // a slot's staging frame: 16 bytes of padding behind the last slot (the second dword of the last window's aligned load)
    static constexpr int chan(int ch) { return 8 * ch; }   // (ba::demosaic: R | G << 8 | B << 16)
    struct Taps { uint32_t r0, r1, r2, r3; };               // the window's four rows
    int w, h;
    int bx, ox0, ox1, px0, px1, by, oy0, oy1, py0, py1;
    __device__ __forceinline__ void place(const TapCols& c) {
        const ba::Axis a = ba::place_axis(c.cx0, c.cx1, w);
        bx = a.origin, ox0 = a.o0, ox1 = a.o1, px0 = a.par0, px1 = a.par1;
    }
    __device__ __forceinline__ void place_rows(int cy0, int cy1) {
        const ba::Axis a = ba::place_axis(cy0, cy1, h);
        by = a.origin, oy0 = a.o0, oy1 = a.o1, py0 = a.par0, py1 = a.par1;
    }
    __device__ __forceinline__ static PlaneGeom plane(const FrontEndGeom& g, int) { return PlaneGeom{g.img_h, g.img_w, 0u}; }
    template <class Source>
    __device__ __forceinline__ Taps fetch(const Source& src, const typename Source::Frame& f, const FrontEndGeom& g, int, int) const {
        const auto p0 = src.plane(f, plane(g, 0), 0);
        return Taps{src.template window<Window>(p0, by, bx), src.template window<Window>(p0, by + 1, bx),
                    src.template window<Window>(p0, by + 2, bx), src.template window<Window>(p0, by + 3, bx)};
    }
    __device__ __forceinline__ void decode(const Taps& t, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) const {
        a0 = ba::window_tap(t.r0, t.r1, t.r2, t.r3, oy0, ox0, ba::phase_of(PATTERN, py0, px0));
        a1 = ba::window_tap(t.r0, t.r1, t.r2, t.r3, oy0, ox1, ba::phase_of(PATTERN, py0, px1));
        b0 = ba::window_tap(t.r0, t.r1, t.r2, t.r3, oy1, ox0, ba::phase_of(PATTERN, py1, px0));
        b1 = ba::window_tap(t.r0, t.r1, t.r2, t.r3, oy1, ox1, ba::phase_of(PATTERN, py1, px1));
    }
};
// a format whose windows depend on the sample's rows beyond cy0 / cy1 as they are says so, and is told them once per walk
template <class F> struct PlacesRows : std::false_type {};
template <int PATTERN> struct PlacesRows<Bayer8<PATTERN>> : std::true_type {};

// Raw Bayer behind a raw table (lt_set_raw_lut; bayer_arith.h: s' = lut[phase][s]): Bayer8 whose 16 window bytes are looked up before
// they reach window_tap -- no extra pass over the frame, no extra byte from it.  The 1 KB table lies in LDS (`lut`), staged by the 256
// threads of the workgroup, one dword each, before any of them leaves the walk.  Window byte (r, c) is site (by + r, bx + c), so rows 0, 2
// and rows 1, 3 of the window have two table rows each: four LDS row bases, frame-independent, found once per walk (place_rows).
template <int PATTERN>
struct Bayer8Lut : Bayer8<PATTERN> {
    typedef Bayer8<PATTERN> Base;
    typedef typename Base::Taps Taps;
    uint8_t* lut;                            // LDS, 1024 bytes
    const uint32_t* table;                   // the context's table, device memory, 256 dwords
    const uint8_t *ea, *eb, *oa, *ob;        // rows 0, 2 of the window: the table rows of columns 0, 2 / 1, 3; rows 1, 3: the same
    __device__ __forceinline__ void stage() const {
        reinterpret_cast<uint32_t*>(lut)[threadIdx.x] = table[threadIdx.x];
        __syncthreads();
    }
    __device__ __forceinline__ void place_rows(int cy0, int cy1) {
        Base::place_rows(cy0, cy1);
        const int py = this->by & 1, px = this->bx & 1;
        ea = lut + ba::lut_row(PATTERN, py, px), eb = lut + ba::lut_row(PATTERN, py, px ^ 1);
        oa = lut + ba::lut_row(PATTERN, py ^ 1, px), ob = lut + ba::lut_row(PATTERN, py ^ 1, px ^ 1);
    }
    __device__ __forceinline__ void decode(const Taps& t, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) const {
        const Taps c{ba::condition4(t.r0, ea, eb), ba::condition4(t.r1, oa, ob), ba::condition4(t.r2, ea, eb), ba::condition4(t.r3, oa, ob)};
        Base::decode(c, a0, a1, b0, b1);
    }
};
template <int PATTERN> struct PlacesRows<Bayer8Lut<PATTERN>> : std::true_type {};
// a format that stages a table in LDS does so before any thread of the workgroup leaves the walk
template <class F> struct StagesTable : std::false_type {};
template <int PATTERN> struct StagesTable<Bayer8Lut<PATTERN>> : std::true_type {};

// 10- / 12-bit raw Bayer (16-bit little-endian words, the sample in the low `bits` bits) behind its wide raw table (lt_set_raw_lut_wide;
// bayer_arith.h: s' = lut[phase][s & mask]): Bayer8's placement, the 4 x 4 window of sites being four 8-byte windows at byte column 2 bx,
// each one aligned 96-bit load (window_at<uint64_t>, as RGB); every site looked up on its way into the four dwords that Bayer8 decodes.
// The table, 4 << bits bytes (4 KB / 16 KB), lies in dynamic LDS, staged by the workgroup's 256 threads in 16-byte pieces before any of
// them leaves the walk.  `bits` is a run-time value: the mask and the table's row stride are scalars.
template <int PATTERN>
struct Bayer16Lut : Bayer8<PATTERN> {
    typedef Bayer8<PATTERN> Base;
    typedef uint64_t Window;
    static constexpr int DENSE_PAD = 16;    // a slot's staging frame: 16 bytes of padding behind the last slot (the third dword of the last window's aligned load)
    struct Taps { uint64_t r0, r1, r2, r3; };               // the window's four rows, four 16-bit sites each
    uint8_t* lut;                            // LDS, 4 << bits bytes
    const uint4* table;                      // the context's table, device memory
    int bits;
    uint32_t mask;                           // (1 << bits) - 1
    const uint8_t *ea, *eb, *oa, *ob;        // as Bayer8Lut's
    __device__ __forceinline__ void stage() const {
        for (int i = threadIdx.x; i < (1 << (bits - 2)); i += 256) reinterpret_cast<uint4*>(lut)[i] = table[i];
        __syncthreads();
    }
    __device__ __forceinline__ void place_rows(int cy0, int cy1) {
        Base::place_rows(cy0, cy1);
        const int py = this->by & 1, px = this->bx & 1;
        ea = lut + ba::lut_row_wide(bits, PATTERN, py, px), eb = lut + ba::lut_row_wide(bits, PATTERN, py, px ^ 1);
        oa = lut + ba::lut_row_wide(bits, PATTERN, py ^ 1, px), ob = lut + ba::lut_row_wide(bits, PATTERN, py ^ 1, px ^ 1);
    }
    __device__ __forceinline__ static PlaneGeom plane(const FrontEndGeom& g, int) { return PlaneGeom{g.img_h, g.img_w * 2, 0u}; }
    template <class Source>
    __device__ __forceinline__ Taps fetch(const Source& src, const typename Source::Frame& f, const FrontEndGeom& g, int, int) const {
        const auto p0 = src.plane(f, plane(g, 0), 0);
        const int col = 2 * this->bx;
        return Taps{src.template window<Window>(p0, this->by, col), src.template window<Window>(p0, this->by + 1, col),
                    src.template window<Window>(p0, this->by + 2, col), src.template window<Window>(p0, this->by + 3, col)};
    }
    __device__ __forceinline__ uint32_t cond(uint64_t r, const uint8_t* a, const uint8_t* b) const {
        return ba::condition4w((uint32_t)r, (uint32_t)(r >> 32), a, b, mask);
    }
    __device__ __forceinline__ void decode(const Taps& t, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) const {
        const typename Base::Taps c{cond(t.r0, ea, eb), cond(t.r1, oa, ob), cond(t.r2, ea, eb), cond(t.r3, oa, ob)};
        Base::decode(c, a0, a1, b0, b1);
    }
};
template <int PATTERN> struct PlacesRows<Bayer16Lut<PATTERN>> : std::true_type {};
template <int PATTERN> struct StagesTable<Bayer16Lut<PATTERN>> : std::true_type {};

// The colour stage of raw Bayer input (lt_set_raw_color; bayer_arith.h: color_px): a wrapper around the two table formats above whose
// decode runs theirs and then takes each of the four demosaiced taps through the colour-correction matrix and the output curve -- before
// the blend, because the clamp and the curve are not linear; the walk masks taps outside the image to 0 afterwards, as ever.  The nine
// coefficients are a kernel argument: wave-uniform, so they stay in SGPRs and every product is a v_mul_i32_i24 / v_mad_i32_i24 with a
// scalar operand (the 16-bit dot form would need the channels packed in pairs first: more instructions, not fewer).  The curve's 256
// bytes lie in LDS right in front of the table -- at a fixed address whatever the table's size; in the 8-bit form, whose LDS is a static
// array, a lookup's offset is an immediate -- and in device memory too (`table`: curve, then table), so that one load per thread and one barrier stage both.
template <int PATTERN>
__device__ __forceinline__ void stage_with_curve(const Bayer8Lut<PATTERN>& f, uint8_t* lds) {        // 1280 bytes: 8 from each of the first 160 threads
    if (threadIdx.x < 160) reinterpret_cast<uint2*>(lds)[threadIdx.x] = reinterpret_cast<const uint2*>(f.table)[threadIdx.x];
    __syncthreads();
}
template <int PATTERN>
__device__ __forceinline__ void stage_with_curve(const Bayer16Lut<PATTERN>& f, uint8_t* lds) {       // 256 + (4 << bits) bytes in 16-byte pieces
    for (int i = threadIdx.x; i < 16 + (1 << (f.bits - 2)); i += 256) reinterpret_cast<uint4*>(lds)[i] = f.table[i];
    __syncthreads();
}
template <class Base>
struct ColorStage : Base {
    typedef typename Base::Taps Taps;
    RawColorMat cm;
    uint8_t* curve;                          // LDS: the curve's 256 bytes, then the table (Base::lut = curve + 256)
    __device__ __forceinline__ void stage() const { stage_with_curve(static_cast<const Base&>(*this), curve); }
    __device__ __forceinline__ void decode(const Taps& t, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) const {
        Base::decode(t, a0, a1, b0, b1);
        a0 = ba::color_px(a0, cm.m, curve), a1 = ba::color_px(a1, cm.m, curve);
        b0 = ba::color_px(b0, cm.m, curve), b1 = ba::color_px(b1, cm.m, curve);
    }
};
template <class B> struct PlacesRows<ColorStage<B>> : PlacesRows<B> {};
template <class B> struct StagesTable<ColorStage<B>> : std::true_type {};

// Lens-shading correction of raw Bayer input (lt_set_raw_shading; shade_arith.h: s' = B + (((s - B) G + 2048) >> 12), clamped): a wrapper
// around the two table formats whose decode shades every site of the 4 x 4 window between its extraction and its table lookup.  The gain
// plane (uint16[h][w], expanded from the mesh by k_shade_expand when the map is set) is fetched like a 16-bit mosaic, but ONCE per walk: the
// window of sites does not depend on the frame, so place_rows loads its four rows -- four aligned 96-bit loads, window_at<uint64_t> -- and
// the 16 gains stay in 8 VGPRs across the per-frame loop.  The four pedestals are a kernel argument (SGPRs); which of them the window's
// even / odd rows and columns have follows from the window's parities, selected once per walk.  Per frame and site: a subtract, a 24-bit
// multiply-add, a shift and a clamp; no vector-memory instruction, no LDS, no scratch.
// (all four read, then selected by value: a select between the ADDRESSES of two members would keep the struct that holds them in scratch)
__device__ __forceinline__ int black_of(const RawShadeBlack& k, int ph) {
    const int b0 = k.b[0], b1 = k.b[1], b2 = k.b[2], b3 = k.b[3];
    const int lo = (ph & 1) ? b1 : b0, hi = (ph & 1) ? b3 : b2;
    return (ph & 2) ? hi : lo;
}
template <class F> struct PatternOf;
template <int P> struct PatternOf<Bayer8Lut<P>> : std::integral_constant<int, P> {};
template <int P> struct PatternOf<Bayer16Lut<P>> : std::integral_constant<int, P> {};
template <class Base>
struct ShadeStage : Base {
    typedef typename Base::Taps Taps;
    static constexpr bool WIDE = sizeof(typename Base::Window) == 8;     // Bayer16Lut: 16-bit sites
    static constexpr int PATTERN = PatternOf<Base>::value;
    __amdgpu_buffer_rsrc_t grs;              // the gain plane and its 16 bytes of padding
    RawShadeBlack blk;
    uint64_t g0, g1, g2, g3;                 // the gains of the window's four rows, four 16-bit gains each
    sa::Black2 ke, ko;                       // the pedestals of rows 0, 2 / 1, 3 of the window (columns 0, 2 and 1, 3)
    __device__ __forceinline__ void shade_with(const uint16_t* gains, const RawShadeBlack& b) {
        grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(gains), 0, __mul24(this->h, this->w) * 2 + 16, RSRC_RAW);
        blk = b;
    }
    __device__ __forceinline__ void place_rows(int cy0, int cy1) {
        Base::place_rows(cy0, cy1);
        const int py = this->by & 1, px = this->bx & 1, pitch = 2 * this->w;
        const uint32_t at = (uint32_t)(__mul24(this->by, pitch) + 2 * this->bx);
        g0 = window_at<uint64_t>(grs, at, 0), g1 = window_at<uint64_t>(grs, at + (uint32_t)pitch, 0);
        g2 = window_at<uint64_t>(grs, at + 2u * (uint32_t)pitch, 0), g3 = window_at<uint64_t>(grs, at + 3u * (uint32_t)pitch, 0);
        ke = sa::black2(black_of(blk, ba::phase_of(PATTERN, py, px)), black_of(blk, ba::phase_of(PATTERN, py, px ^ 1)));
        ko = sa::black2(black_of(blk, ba::phase_of(PATTERN, py ^ 1, px)), black_of(blk, ba::phase_of(PATTERN, py ^ 1, px ^ 1)));
    }
    template <class Row>
    __device__ __forceinline__ uint32_t cond(Row r, uint64_t g, const sa::Black2& k, const uint8_t* a, const uint8_t* b) const {
        if constexpr (WIDE) return sa::shade_condition4w((uint32_t)r, (uint32_t)(r >> 32), (uint32_t)g, (uint32_t)(g >> 32), k, a, b, this->mask);
        else return sa::shade_condition4(r, (uint32_t)g, (uint32_t)(g >> 32), k, a, b);
    }
    __device__ __forceinline__ void decode(const Taps& t, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) const {
        const typename Bayer8<PATTERN>::Taps c{cond(t.r0, g0, ke, this->ea, this->eb), cond(t.r1, g1, ko, this->oa, this->ob),
                                               cond(t.r2, g2, ke, this->ea, this->eb), cond(t.r3, g3, ko, this->oa, this->ob)};
        Bayer8<PATTERN>::decode(c, a0, a1, b0, b1);
    }
};
template <class B> struct PlacesRows<ShadeStage<B>> : std::true_type {};
template <class B> struct StagesTable<ShadeStage<B>> : std::true_type {};

// MIPI-packed RAW10 / RAW12 (mipi_arith.h; PACK 0: five bytes for four sites, 1: three bytes for two) in front of Bayer16Lut, shaded or not:
// Bayer8's placement once more, the 4 x 4 window of sites being four windows of at most 9 / 8 bytes from byte first_byte(bx) of their rows --
// each the one aligned 96-bit load of the 16-bit walk, at any byte alignment of the row -- and every window row unpacked into the four 16-bit
// words that Inner decodes.  Which bytes and bits of a window hold its four samples depends on bx alone: the selectors and shifts are found
// once per walk (place), and a frame adds byte permutes, packed shifts and ors -- no memory instruction, no LDS access.  Table, dynamic LDS,
// staging, mask and lookups are Inner's: the samples have no bits above `bits`, so the mask changes nothing.
template <int PACK, class Inner>
struct MipiUnpack : Inner {
    typedef std::conditional_t<PACK == ma::PACK10, Bytes12, uint64_t> Window;
    struct Row { uint32_t w0, w1, w2; };                    // (w2: RAW10 only)
    struct Taps { Row r0, r1, r2, r3; };
    ma::Unpack up;
    int col;
    __device__ __forceinline__ void place(const TapCols& c) {
        Inner::place(c);
        up = ma::unpack_of(PACK, this->bx);
        col = ma::first_byte(PACK, this->bx);
    }
    __device__ __forceinline__ static PlaneGeom plane(const FrontEndGeom& g, int) { return PlaneGeom{g.img_h, ma::row_bytes(PACK, g.img_w), 0u}; }
    template <class Source, class Plane>
    __device__ __forceinline__ Row row_at(const Source& src, const Plane& p0, int row) const {
        const Window w = src.template window<Window>(p0, row, col);
        if constexpr (PACK == ma::PACK10) return Row{w.w0, w.w1, w.w2};
        else return Row{(uint32_t)w, (uint32_t)(w >> 32), 0u};
    }
    template <class Source>
    __device__ __forceinline__ Taps fetch(const Source& src, const typename Source::Frame& f, const FrontEndGeom& g, int, int) const {
        const auto p0 = src.plane(f, plane(g, 0), 0);
        return Taps{row_at(src, p0, this->by), row_at(src, p0, this->by + 1), row_at(src, p0, this->by + 2), row_at(src, p0, this->by + 3)};
    }
    __device__ __forceinline__ uint64_t words(const Row& r) const {
        uint32_t lo, hi;
        ma::samples4<PACK>(up, r.w0, r.w1, r.w2, lo, hi);
        return (uint64_t)lo | ((uint64_t)hi << 32);
    }
    __device__ __forceinline__ void decode(const Taps& t, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) const {
        const typename Inner::Taps c{words(t.r0), words(t.r1), words(t.r2), words(t.r3)};
        Inner::decode(c, a0, a1, b0, b1);
    }
};
template <int K, class I> struct PlacesRows<MipiUnpack<K, I>> : std::true_type {};
template <int K, class I> struct StagesTable<MipiUnpack<K, I>> : std::true_type {};

// The slots' own frames: `stride` bytes apart, planes dense.  One buffer resource covers the frames [z0, z1) of the walk (a frame
// is selected by the scalar offset of the load) plus the format's padding behind them; beyond that the resource returns 0.
// 32-bit offsets (a walk stays below 2^30 bytes: launch_undistort_rows) keep the address math on full-rate 24-bit multiplies.
// ALIGNED4 = false, for frames or strides that are not 4-byte aligned: a plain unaligned load of the window (8-byte windows only).
template <bool ALIGNED4>
struct SlotSource {
    typedef int Frame;                       // byte offset of a frame behind the first of the walk
    const uint8_t* frames;                   // frame 0 of the launch
    size_t stride;
    const uint8_t* base;                     // frame z0
    int z0;
    __amdgpu_buffer_rsrc_t rs;
    __device__ __forceinline__ void begin(int, int z0_, int z1, int pad) {
        base = frames + (size_t)z0_ * stride;
        z0 = z0_;
        rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0, (z1 - z0_) * (int)stride + pad, RSRC_RAW);
    }
    __device__ __forceinline__ Frame frame(int z) const { return (z - z0) * (int)stride; }
    struct Plane { uint32_t first; int pitch; Frame f; };
    __device__ __forceinline__ Plane plane(const Frame& f, const PlaneGeom& pg, int) const { return Plane{pg.dense, pg.row_bytes, f}; }
    template <class W>
    __device__ __forceinline__ W window(const Plane& pl, int row, int col) const {
        const uint32_t off = pl.first + (uint32_t)(__mul24(row, pl.pitch) + col);
        if constexpr (ALIGNED4) {
            return window_at<W>(rs, off, pl.f);
        } else {
            struct __attribute__((packed, aligned(1))) Unaligned { W v; };
            return reinterpret_cast<const Unaligned*>(base + (size_t)(unsigned)pl.f + off)->v;
        }
    }
    // an 8-byte window at a column that is a multiple of 4 in a plane whose pitch is one too: the two dwords as they lie
    __device__ __forceinline__ uint64_t dwords2(const Plane& pl, int row, int col) const {
        if constexpr (ALIGNED4) {
            const u32x2 d = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(pl.first + (uint32_t)(__mul24(row, pl.pitch) + col)), pl.f, 0);
            return (uint64_t)d.x | ((uint64_t)d.y << 32);
        } else {
            return window<uint64_t>(pl, row, col);
        }
    }
};

// Frames that lie in the caller's device memory (lt_attach_device_frames): entry first_slot + z of the surface table (device
// memory, SurfEntry per slot) holds the plane pointers and pitches of frame z.  z is wave-uniform, so an entry arrives by scalar
// loads and every plane gets a buffer resource of its own in SGPRs, based at ptr & ~3 -- the remainder goes into the windows'
// offsets, which are split into an aligned load and a v_alignbyte_b32 anyway -- and covering exactly the plane's bytes, rounded up
// to the end of the aligned dword that holds its last byte: pitch * (rows - 1) + row bytes.  A window that overruns the plane
// comes back as zeros from the resource's range check (raw buffers are checked dword by dword) and those bytes are never used;
// nothing is read outside the dwords the plane occupies, so a surface may end on the last byte of its allocation.
struct SurfPlane { __amdgpu_buffer_rsrc_t rs; int rem, pitch; };
__device__ __forceinline__ SurfPlane surf_plane(uint64_t ptr, int pitch, int rows, int row_bytes) {
    const int rem = (int)(ptr & 3u);
    return SurfPlane{__builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(ptr & ~(uint64_t)3), 0,
                                                       (rem + __mul24(pitch, rows - 1) + row_bytes + 3) & ~3, RSRC_RAW), rem, pitch};
}
struct SurfSource {
    typedef SurfEntry Frame;
    const SurfEntry* tab;
    const SurfEntry* ent;                    // entry of frame 0 of the launch
    __device__ __forceinline__ void begin(int first_slot, int, int, int) { ent = tab + first_slot; }
    __device__ __forceinline__ Frame frame(int z) const { return ent[z]; }
    typedef SurfPlane Plane;
    __device__ __forceinline__ Plane plane(const Frame& e, const PlaneGeom& pg, int p) const {
        return surf_plane(e.plane[p], p == 0 ? e.pitch : e.cpitch, pg.rows, pg.row_bytes);
    }
    // pitch and remainder are the frame's, so the offset is too
    template <class W>
    __device__ __forceinline__ W window(const Plane& pl, int row, int col) const {
        return window_at<W>(pl.rs, (uint32_t)(__mul24(row, pl.pitch) + col + pl.rem), 0);
    }
    // (a surface lies at any byte: nothing is known of the window's alignment)
    __device__ __forceinline__ uint64_t dwords2(const Plane& pl, int row, int col) const { return window<uint64_t>(pl, row, col); }
};

// Whose remap table a walk reads: the launch's one table (a.uxy, a.ufrac), or -- PER_SLOT, the table-per-slot form, one frame per
// walk -- that of the calibration set of the walk's slot (a.tabs).  The slot is wave-uniform, so its set's id (a byte of the
// kernel argument) and the set's entry of the set table (device memory) arrive by scalar loads, as a surface's entry does.
struct SlotTables {
    const CalTables* sets;
    const CalIds* ids;
    __device__ __forceinline__ const CalTables& of(int z) const { return sets[(ids->w[z >> 2] >> (8 * (z & 3))) & 255u]; }
};

// What the kernels below hand to the walk besides their source and format.
struct WalkArgs {
    const int16_t* uxy;
    const uint16_t* ufrac;
    SlotTables tabs;
    FrontEndGeom g;
    uint32_t* und;
    size_t und_px;
    int first_slot, n, fpb, remap;
};

template <bool PER_SLOT, class Source, class Format>
__device__ __forceinline__ void undistort_walk(const WalkArgs& a, Source src, Format fmt) {
    const FrontEndGeom& g = a.g;
    const uint32_t per_z = gridDim.x * gridDim.y;
    const uint32_t id = xcd_block((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, per_z * gridDim.z, a.remap);
    const uint32_t bz = id / per_z, by = (id - bz * per_z) / gridDim.x, bx = id - bz * per_z - by * gridDim.x;
    // (blockDim.x of a __global__ function: written as blockDim.x here, in a device function, it is lowered through the generic
    // work-group-size path -- a third v_mul_lo_u32 and a global_load_ushort in the prologue)
    const int x = bx * __builtin_amdgcn_workgroup_size_x() + threadIdx.x;
    const int row = by;  // relative to g.r0
    if constexpr (StagesTable<Format>::value) fmt.stage();
    if (x >= g.img_w) return;
    const int z0 = bz * a.fpb, z1 = min(z0 + a.fpb, a.n);   // fpb frames per thread: table entry and offsets are frame-independent
    const size_t o = (size_t)row * g.img_w + x;
    const int16_t* uxy = a.uxy;
    const uint16_t* ufrac = a.ufrac;
    if constexpr (PER_SLOT) {                // (fpb == 1: the walk is slot first_slot + z0's)
        const CalTables& t = a.tabs.of(z0);
        uxy = t.uxy;
        ufrac = t.ufrac;
    }
    const int sx = uxy[o * 2], sy = uxy[o * 2 + 1];
    const int f = ufrac[o], fx = f & 31, fy = f >> 5;
    const bool y0 = sy >= 0 && sy < g.img_h, y1 = sy + 1 >= 0 && sy + 1 < g.img_h;
    const bool x0 = sx >= 0 && sx < g.img_w, x1 = sx + 1 >= 0 && sx + 1 < g.img_w;
    const int cy0 = min(max(sy, 0), g.img_h - 1), cy1 = min(max(sy + 1, 0), g.img_h - 1);
    const TapCols cols{min(max(sx, 0), g.img_w - 2), min(max(sx, 0), g.img_w - 1), min(max(sx + 1, 0), g.img_w - 1)};
    fmt.place(cols);
    if constexpr (PlacesRows<Format>::value) fmt.place_rows(cy0, cy1);
    const uint32_t m00 = (y0 && x0) ? 255u : 0u, m01 = (y0 && x1) ? 255u : 0u;
    const uint32_t m10 = (y1 && x0) ? 255u : 0u, m11 = (y1 && x1) ? 255u : 0u;
    const uint32_t gx = 32u - (uint32_t)fx, gy = 32u - (uint32_t)fy;
    const uint32_t w00 = (gx * gy) & 0x7ffu, w01 = ((uint32_t)fx * gy) & 0x7ffu, w10 = (gx * (uint32_t)fy) & 0x7ffu, w11 = ((uint32_t)fx * (uint32_t)fy) & 0x7ffu;
    // the slots this thread writes: pairs [pair0, pair1] of the interleaved buffer
    const int pair0 = (a.first_slot + z0) >> 1, pair1 = (a.first_slot + z1 - 1) >> 1, pair_b = (int)(a.und_px * 8);
    const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(a.und + (size_t)pair0 * 2 * a.und_px, 0, (pair1 - pair0 + 1) * pair_b, RSRC_RAW);
    src.begin(a.first_slot, z0, z1, Format::DENSE_PAD);
    auto fr = src.frame(z0);
    auto q = fmt.fetch(src, fr, g, cy0, cy1);
    fr = src.frame(min(z0 + 1, z1 - 1));
    for (int z = z0; z < z1; ++z) {
        // the next frame's windows are in flight while this one is (converted and) blended, and the frame after it is being located
        // (surfaces: its entry is on its way)
        const auto nq = fmt.fetch(src, fr, g, cy0, cy1);
        fr = src.frame(min(z + 2, z1 - 1));
        uint32_t a0, a1, b0, b1;
        fmt.decode(q, a0, a1, b0, b1);
        uint32_t out = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t v00 = (a0 >> Format::chan(ch)) & m00, v01 = (a1 >> Format::chan(ch)) & m01;
            const uint32_t v10 = (b0 >> Format::chan(ch)) & m10, v11 = (b1 >> Format::chan(ch)) & m11;
            // (sum_i w_i p_i + 2^9) >> 10: the same integer as bilerp(); with the 11-bit weights visible every product is a
            // v_mul_u32_u24 / v_mad_u32_u24 (the two-stage form was re-associated into quarter-rate 32- and 64-bit multiplies)
            out |= ((v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + 512u) >> 10) << (8 * ch);
            // Opaque to the optimiser, free at run time: it keeps the third channel from being re-associated into the OR of the
            // first two (which happens once this unrolled loop is inlined into a kernel), after which the two v_and_or_b32 of the
            // packing are selected as two v_and_b32 + a v_or3_b32 -- one VALU instruction more per frame, two more VGPRs in the
            // 4:2:0 surface walks.
            if (ch == 1) asm("" : "+v"(out));
        }
        const int slot = a.first_slot + z;   // wave-uniform: pair and parity go into the scalar offset of the store
        __builtin_amdgcn_raw_buffer_store_b32(out, urs, (int)o * 8, __builtin_amdgcn_readfirstlane(((slot >> 1) - pair0) * pair_b + (slot & 1) * 4), 0);
        q = nq;
    }
}

// The layout of a frame (lt_internal.h: launch_undistort_rows) as the walk's pixel format -- the one place where the number becomes a type.
template <int LAYOUT>
__device__ __forceinline__ auto format_of(const FrontEndGeom& g, const YuvCoef& k) {
    if constexpr (LAYOUT == 0) return Rgb24{};
    else if constexpr (LAYOUT <= 2) return Yuv420<LAYOUT>{k};
    else if constexpr (LAYOUT <= 4) return Yuv422<LAYOUT - 3>{k, (g.img_w >> 1) - 2};
    else if constexpr (LAYOUT <= 7) return PxFormat<LAYOUT>{};
    else return Bayer8<LAYOUT - 16>{g.img_w, g.img_h};
}

// The walk's one entry point: layout x source x table form.  SRC: where the frames lie -- the caller's surfaces (`tab`), or the slots'
// own frames (`frames`, `stride`) at a dword-aligned base and stride or at any byte (plain RGB only; a staging frame of every other
// layout is dword-aligned: lt_set_input_format).  PER_SLOT: the table-per-slot form (a context whose slots hold cameras of different
// calibrations: a slice that mixes sets) -- one frame per walk, with the tables sets[id] of its slot, `ids`: the sets of slots
// first_slot, first_slot + 1, ...; else the launch's one table uxy / ufrac and fpb frames per walk.  Every form has the same parameter
// list and reads what it needs: `k` the YUV layouts.  (The name is what the profiles and tools know the walks by.)
constexpr int SRC_SURFACES = 0, SRC_SLOTS = 1, SRC_SLOTS_ANY_BYTE = 2;
template <int LAYOUT, int SRC, bool PER_SLOT>
__global__ __launch_bounds__(256) void k_undistort_rows(const SurfEntry* __restrict__ tab, const uint8_t* __restrict__ frames, size_t stride,
                                                       YuvCoef k, const int16_t* __restrict__ uxy, const uint16_t* __restrict__ ufrac,
                                                       const CalTables* __restrict__ sets, CalIds ids, FrontEndGeom g,
                                                       uint32_t* __restrict__ und, size_t und_px, int first_slot, int n, int fpb, int remap) {
    static_assert(SRC != SRC_SLOTS_ANY_BYTE || LAYOUT == 0, "only plain RGB frames lie at any byte");
    const WalkArgs a{uxy, ufrac, SlotTables{sets, &ids}, g, und, und_px, first_slot, n, PER_SLOT ? 1 : fpb, remap};
    if constexpr (SRC == SRC_SURFACES) undistort_walk<PER_SLOT>(a, SurfSource{tab}, format_of<LAYOUT>(g, k));
    else undistort_walk<PER_SLOT>(a, SlotSource<SRC == SRC_SLOTS>{frames, stride}, format_of<LAYOUT>(g, k));
}

// The walk over raw Bayer frames behind a raw table: PATTERN x source (surfaces, dword-aligned slots) x table form x STAGES -- bit 0: 16-bit
// samples behind the wide table (else bytes), bit 1: the colour stage on every demosaiced tap, bit 2: the shading map in front of the
// lookup.  k_undistort_rows' parameters without `k`, and what the stages read (lt_internal.h: RawStages; a member that a form does not
// read is never loaded).  r.table is what the workgroup stages: the table, behind the curve's 256 bytes with a colour stage -- 1024 (+ 256)
// bytes of static LDS for 8-bit samples, so that a lookup's offset is an immediate, the launch's dynamic LDS, 4 << bits (+ 256), for 16-bit
// ones.  Launched in k_undistort_rows' place, in the same stage, whenever there is a table -- the identity included.
template <int PATTERN, bool W16, bool CC, bool LS>
struct RawFormatOf {
    using Base = std::conditional_t<W16, Bayer16Lut<PATTERN>, Bayer8Lut<PATTERN>>;
    using Shaded = std::conditional_t<LS, ShadeStage<Base>, Base>;
    using type = std::conditional_t<CC, ColorStage<Shaded>, Shaded>;
};
extern __shared__ __attribute__((aligned(16))) uint8_t s_lut_wide[];
// where a raw kernel stages: the launch's dynamic LDS (16-bit samples) or CURVE + 1024 bytes of static LDS
template <bool W16, int CURVE>
__device__ __forceinline__ uint8_t* raw_lds() {
    if constexpr (W16) {
        return s_lut_wide;
    } else {
        __shared__ alignas(16) uint8_t s_tab[CURVE + 1024];
        return s_tab;
    }
}
// the bodies of the raw walks: the format of STAGES made of `r`, then the one walk.  Shared by the kernels that are given `r` and by those
// that find it in their slot's raw set (k_rawset_walk_rows, k_packset_walk_rows)
template <int PATTERN, int SRC, bool PER_SLOT, int STAGES>
__device__ __forceinline__ void raw_walk(const WalkArgs& a, uint8_t* lds, const SurfEntry* __restrict__ tab, const uint8_t* __restrict__ frames,
                                         size_t stride, const RawStages& r) {
    constexpr bool W16 = (STAGES & 1) != 0, CC = (STAGES & 2) != 0, LS = (STAGES & 4) != 0;
    constexpr int CURVE = CC ? 256 : 0;
    const FrontEndGeom& g = a.g;
    typename RawFormatOf<PATTERN, W16, CC, LS>::type fmt{};
    fmt.w = g.img_w, fmt.h = g.img_h, fmt.lut = lds + CURVE;
    if constexpr (W16) fmt.table = reinterpret_cast<const uint4*>(r.table), fmt.bits = r.bits, fmt.mask = (1u << r.bits) - 1u;
    else fmt.table = r.table;
    if constexpr (CC) fmt.cm = r.cm, fmt.curve = lds;
    if constexpr (LS) fmt.shade_with(r.gains, r.blk);
    if constexpr (SRC == SRC_SURFACES) undistort_walk<PER_SLOT>(a, SurfSource{tab}, fmt);
    else undistort_walk<PER_SLOT>(a, SlotSource<true>{frames, stride}, fmt);
}
template <int PATTERN, int SRC, bool PER_SLOT, int STAGES, int PACK>
__device__ __forceinline__ void mipi_walk(const WalkArgs& a, const SurfEntry* __restrict__ tab, const uint8_t* __restrict__ frames, size_t stride,
                                          const RawStages& r) {
    static_assert((STAGES & 1) != 0, "packed samples are 10 / 12 bits wide: behind the wide table");
    constexpr bool CC = (STAGES & 2) != 0, LS = (STAGES & 4) != 0;
    constexpr int CURVE = CC ? 256 : 0;
    uint8_t* lds = s_lut_wide;
    const FrontEndGeom& g = a.g;
    using Unpacked = MipiUnpack<PACK, std::conditional_t<LS, ShadeStage<Bayer16Lut<PATTERN>>, Bayer16Lut<PATTERN>>>;
    std::conditional_t<CC, ColorStage<Unpacked>, Unpacked> fmt{};
    fmt.w = g.img_w, fmt.h = g.img_h, fmt.lut = lds + CURVE;
    fmt.table = reinterpret_cast<const uint4*>(r.table), fmt.bits = r.bits, fmt.mask = (1u << r.bits) - 1u;
    if constexpr (CC) fmt.cm = r.cm, fmt.curve = lds;
    if constexpr (LS) fmt.shade_with(r.gains, r.blk);
    if constexpr (SRC == SRC_SURFACES) undistort_walk<PER_SLOT>(a, SurfSource{tab}, fmt);
    else undistort_walk<PER_SLOT>(a, SlotSource<true>{frames, stride}, fmt);
}
template <int PATTERN, int SRC, bool PER_SLOT, int STAGES>
__global__ __launch_bounds__(256) void k_raw_walk_rows(const SurfEntry* __restrict__ tab, const uint8_t* __restrict__ frames, size_t stride,
                                                      const int16_t* __restrict__ uxy, const uint16_t* __restrict__ ufrac,
                                                      const CalTables* __restrict__ sets, CalIds ids, FrontEndGeom g,
                                                      uint32_t* __restrict__ und, size_t und_px, int first_slot, int n, int fpb, int remap,
                                                      RawStages r) {
    static_assert(SRC == SRC_SURFACES || SRC == SRC_SLOTS, "a raw Bayer staging frame is dword-aligned");
    constexpr bool W16 = (STAGES & 1) != 0, CC = (STAGES & 2) != 0;
    const WalkArgs a{uxy, ufrac, SlotTables{sets, &ids}, g, und, und_px, first_slot, n, PER_SLOT ? 1 : fpb, remap};
    raw_walk<PATTERN, SRC, PER_SLOT, STAGES>(a, raw_lds<W16, CC ? 256 : 0>(), tab, frames, stride, r);
}

// ... over MIPI-packed RAW10 / RAW12 frames (PACK; mipi_arith.h): k_raw_walk_rows' 16-bit forms (STAGES 1, 3, 5, 7) with every window row
// unpacked on its way in -- the same parameters, the same dynamic LDS, r.bits = 10 / 12 as PACK says.
template <int PATTERN, int SRC, bool PER_SLOT, int STAGES, int PACK>
__global__ __launch_bounds__(256) void k_mipi_walk_rows(const SurfEntry* __restrict__ tab, const uint8_t* __restrict__ frames, size_t stride,
                                                       const int16_t* __restrict__ uxy, const uint16_t* __restrict__ ufrac,
                                                       const CalTables* __restrict__ sets, CalIds ids, FrontEndGeom g,
                                                       uint32_t* __restrict__ und, size_t und_px, int first_slot, int n, int fpb, int remap,
                                                       RawStages r) {
    static_assert(SRC == SRC_SURFACES || SRC == SRC_SLOTS, "a raw Bayer staging frame is dword-aligned");
    const WalkArgs a{uxy, ufrac, SlotTables{sets, &ids}, g, und, und_px, first_slot, n, PER_SLOT ? 1 : fpb, remap};
    mipi_walk<PATTERN, SRC, PER_SLOT, STAGES, PACK>(a, tab, frames, stride, r);
}

// The set-per-slot forms of the two walks above, for a launch whose slots mix raw sets (lt_add_raw_set): a workgroup serves ONE slot -- the
// table-per-slot geometry, one frame per walk, which these forms always have for the calibration as well -- and takes what the one-set
// kernels take as `r` from its slot's entry of the table of raw sets (raw_setup.h: RawSetEntry).  The slot is wave-uniform, so its set's id
// (a byte of the kernel argument `rids`, as CalIds) and the 80 bytes of the entry arrive by scalar loads: the staged-bytes pointer, which the
// workgroup then stages THAT set's table (and curve) from, the gain plane's pointer, which the shading stage builds its resource from, the
// matrix and the pedestals, which stay in SGPRs.  STAGES is the union of the parts the context's sets have; a set that lacks one has its
// identity in its entry.  Behind that prologue the walk is the walk of the one-set form, instruction for instruction.
__device__ __forceinline__ int walk_slot_z(int remap) {          // undistort_walk's bz (fpb == 1: the walk's frame)
    const uint32_t per_z = gridDim.x * gridDim.y;
    return (int)(xcd_block((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, per_z * gridDim.z, remap) / per_z);
}
__device__ __forceinline__ RawStages stages_of_set(const RawSetEntry* __restrict__ rsets, const CalIds& rids, int z, int bits) {
    const RawSetEntry& e = rsets[__builtin_amdgcn_readfirstlane((rids.w[z >> 2] >> (8 * (z & 3))) & 255u)];
    RawStages r;
    r.table = e.table, r.bits = bits, r.cm = e.cm, r.gains = e.gains, r.blk = e.blk;
    return r;
}
template <int PATTERN, int SRC, int STAGES>
__global__ __launch_bounds__(256) void k_rawset_walk_rows(const SurfEntry* __restrict__ tab, const uint8_t* __restrict__ frames, size_t stride,
                                                         const CalTables* __restrict__ sets, CalIds ids, FrontEndGeom g,
                                                         uint32_t* __restrict__ und, size_t und_px, int first_slot, int n, int remap,
                                                         const RawSetEntry* __restrict__ rsets, CalIds rids, int bits) {
    constexpr bool W16 = (STAGES & 1) != 0, CC = (STAGES & 2) != 0;
    const WalkArgs a{nullptr, nullptr, SlotTables{sets, &ids}, g, und, und_px, first_slot, n, 1, remap};
    raw_walk<PATTERN, SRC, true, STAGES>(a, raw_lds<W16, CC ? 256 : 0>(), tab, frames, stride, stages_of_set(rsets, rids, walk_slot_z(remap), bits));
}
template <int PATTERN, int SRC, int STAGES, int PACK>
__global__ __launch_bounds__(256) void k_packset_walk_rows(const SurfEntry* __restrict__ tab, const uint8_t* __restrict__ frames, size_t stride,
                                                          const CalTables* __restrict__ sets, CalIds ids, FrontEndGeom g,
                                                          uint32_t* __restrict__ und, size_t und_px, int first_slot, int n, int remap,
                                                          const RawSetEntry* __restrict__ rsets, CalIds rids, int bits) {
    const WalkArgs a{nullptr, nullptr, SlotTables{sets, &ids}, g, und, und_px, first_slot, n, 1, remap};
    mipi_walk<PATTERN, SRC, true, STAGES, PACK>(a, tab, frames, stride, stages_of_set(rsets, rids, walk_slot_z(remap), bits));
}

// The expansion of a shading mesh (uint16[4][mh][mw], device memory) into the gain plane of an h x w image with `pattern`: one thread per
// site, shade_arith.h's gain_at.  A set-up kernel (lt_set_raw_shading), so its one integer division per axis is left as it is.
__global__ __launch_bounds__(256) void k_shade_expand(const uint16_t* __restrict__ mesh, int mw, int mh, int pattern, uint16_t* __restrict__ plane, int h, int w) {
    const int x = (int)(blockIdx.x * 256 + threadIdx.x), y = (int)blockIdx.y;
    if (x >= w) return;
    plane[(size_t)y * w + x] = (uint16_t)sa::gain_at(mesh + (size_t)ba::phase(pattern, y, x) * mh * mw, mw, mh, y, x, h, w);
}

// ---- camera rows -> RGB rows ---------------------------------------------------------------------------------------------------
// Rows [r0, r1) of frames in another layout -> the same rows of RGB frames (3 B/px): a streaming kernel for whoever shows the camera
// frame.  Per family of layouts a description (Rows420, Rows422, RowsPx, RowsBayer) holds what its conversion is made of:
//   wide         the body of a thread that owns the 16 columns from x0: 16-byte loads, 48 bytes per row in three 16-byte stores (for a
//                width and every base and pitch that are multiples of 16)
//   any          the body for any width, any pitch and any alignment, byte accesses: thread i owns the ANY_COLS columns from ANY_COLS * i
//   CHROMA_ROWS  a launch row `row` is a chroma row, the frame rows 2 row and 2 row + 1 (4:2:0); else the frame row itself
//   dense        the planes of a slot's dense staging frame (a surface's planes and pitches: its entry)
// Both bodies take (planes, k, dst frame, h, w, r0, r1, row, x0 or i).
struct Planes {
    const uint8_t *y, *u, *v;                // y: the one plane of a single-plane layout; u: NV12's plane of (U, V) pairs; v: I420 only
    int pitch, cpitch;
};
__device__ __forceinline__ Planes surf_planes(const SurfEntry& e) {
    return Planes{reinterpret_cast<const uint8_t*>(e.plane[0]), reinterpret_cast<const uint8_t*>(e.plane[1]),
                  reinterpret_cast<const uint8_t*>(e.plane[2]), e.pitch, e.cpitch};
}

// The tail of the wide bodies: four pixels (R | G << 8 | B << 16) -> the three dwords of their 12 bytes, and the twelve dwords of 16
// pixels -> 48 bytes at `at` in three 16-byte stores
__device__ __forceinline__ void pack_rgb4(const uint32_t* px, uint32_t* d) {
    d[0] = px[0] | (px[1] << 24);
    d[1] = (px[1] >> 8) | (px[2] << 16);
    d[2] = (px[2] >> 16) | (px[3] << 8);
}
__device__ __forceinline__ void store_rgb16(uint8_t* at, const uint32_t (&d)[12]) {
    uint4* o = reinterpret_cast<uint4*>(at);
    o[0] = make_uint4(d[0], d[1], d[2], d[3]);
    o[1] = make_uint4(d[4], d[5], d[6], d[7]);
    o[2] = make_uint4(d[8], d[9], d[10], d[11]);
}
__device__ __forceinline__ void store_rgb1(uint8_t* at, uint32_t px) {
    at[0] = (uint8_t)px;
    at[1] = (uint8_t)(px >> 8);
    at[2] = (uint8_t)(px >> 16);
}

// 4:2:0 (LAYOUT 1: NV12, 2: I420).
template <int LAYOUT>
struct Rows420 {
    static constexpr bool CHROMA_ROWS = true;
    static constexpr int ANY_COLS = 2;
    __device__ __forceinline__ static Planes dense(const uint8_t* frame, int h, int w) {
        const size_t plane = (size_t)h * w;
        return Planes{frame, frame + plane, frame + plane + (plane >> 2), w, LAYOUT == 1 ? w : w >> 1};
    }
    // The two rows of chroma row `cr`: 16 Y bytes per row and the 8 (U, V) pairs under them in 16-byte loads, each pair's three chroma
    // terms computed once for its four pixels.  Either row of the pair may lie outside [r0, r1) (block-uniform) and is then neither
    // read nor written.
    __device__ __forceinline__ static void wide(const Planes& p, YuvCoef k, uint8_t* dst, int, int w, int r0, int r1, int cr, int x0) {
        if (x0 >= w) return;
        uint32_t uv[4];                                    // NV12: 8 (U, V) pairs; I420: uv[0..1] 8 U, uv[2..3] 8 V
        if constexpr (LAYOUT == 1) {
            const uint4 c = *reinterpret_cast<const uint4*>(p.u + (size_t)cr * p.cpitch + x0);
            uv[0] = c.x; uv[1] = c.y; uv[2] = c.z; uv[3] = c.w;
        } else {
            const size_t co = (size_t)cr * p.cpitch + (x0 >> 1);
            const uint2 cu = *reinterpret_cast<const uint2*>(p.u + co), cv = *reinterpret_cast<const uint2*>(p.v + co);
            uv[0] = cu.x; uv[1] = cu.y; uv[2] = cv.x; uv[3] = cv.y;
        }
        Chroma c[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int u, v;
            if constexpr (LAYOUT == 1) {
                u = (int)((uv[i >> 1] >> (16 * (i & 1))) & 255u);
                v = (int)((uv[i >> 1] >> (16 * (i & 1) + 8)) & 255u);
            } else {
                u = (int)((uv[i >> 2] >> (8 * (i & 3))) & 255u);
                v = (int)((uv[2 + (i >> 2)] >> (8 * (i & 3))) & 255u);
            }
            c[i] = yuv_chroma(u, v, k);
        }
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * cr + dy;
            if (y < r0 || y >= r1) continue;
            const uint4 yq = *reinterpret_cast<const uint4*>(p.y + (size_t)y * p.pitch + x0);
            const uint32_t yw[4] = {yq.x, yq.y, yq.z, yq.w};
            uint32_t d[12];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                  // four pixels (two chroma pairs) -> three dwords
                uint32_t px[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) px[i] = yuv_pixel((int)((yw[j] >> (8 * i)) & 255u), c[2 * j + (i >> 1)], k);
                pack_rgb4(px, d + 3 * j);
            }
            store_rgb16(dst + ((size_t)y * w + x0) * 3, d);
        }
    }
    // one thread per 2 x 2 block (block column bx)
    __device__ __forceinline__ static void any(const Planes& p, YuvCoef k, uint8_t* dst, int, int w, int r0, int r1, int cr, int bx) {
        if (2 * bx >= w) return;
        int u, v;
        if constexpr (LAYOUT == 1) {
            u = p.u[(size_t)cr * p.cpitch + 2 * bx];
            v = p.u[(size_t)cr * p.cpitch + 2 * bx + 1];
        } else {
            u = p.u[(size_t)cr * p.cpitch + bx];
            v = p.v[(size_t)cr * p.cpitch + bx];
        }
        const Chroma c = yuv_chroma(u, v, k);
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * cr + dy;
            if (y < r0 || y >= r1) continue;
            for (int dx = 0; dx < 2; ++dx)
                store_rgb1(dst + ((size_t)y * w + 2 * bx + dx) * 3, yuv_pixel(p.y[(size_t)y * p.pitch + 2 * bx + dx], c, k));
        }
    }
};

// Packed 4:2:2 (ORDER 0: YUY2, 1: UYVY): row y of the one plane -> row y of the RGB frame.
template <int ORDER>
struct Rows422 {
    static constexpr bool CHROMA_ROWS = false;
    static constexpr int ANY_COLS = 2;
    __device__ __forceinline__ static Planes dense(const uint8_t* frame, int, int w) { return Planes{frame, nullptr, nullptr, 2 * w, 0}; }
    // 8 macropixels in two 16-byte loads, each macropixel's three chroma terms computed once for its two pixels
    __device__ __forceinline__ static void wide(const Planes& s, YuvCoef k, uint8_t* dst, int, int w, int, int, int y, int x0) {
        if (x0 >= w) return;
        const uint4* in = reinterpret_cast<const uint4*>(s.y + (size_t)y * s.pitch + 2 * x0);
        const uint4 q0 = in[0], q1 = in[1];
        const uint32_t m[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        uint32_t d[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                      // two macropixels (four pixels) -> three dwords
            uint32_t px[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t mp = m[2 * j + i];
                const Chroma c = yuv_chroma((int)((mp >> ya::ush422(ORDER)) & 255u), (int)((mp >> ya::vsh422(ORDER)) & 255u), k);
                px[2 * i] = yuv_pixel((int)((mp >> ya::ysh422(ORDER, 0)) & 255u), c, k);
                px[2 * i + 1] = yuv_pixel((int)((mp >> ya::ysh422(ORDER, 1)) & 255u), c, k);
            }
            pack_rgb4(px, d + 3 * j);
        }
        store_rgb16(dst + ((size_t)y * w + x0) * 3, d);
    }
    // one thread per macropixel (index mx of row y)
    __device__ __forceinline__ static void any(const Planes& s, YuvCoef k, uint8_t* dst, int, int w, int, int, int y, int mx) {
        if (2 * mx >= w) return;
        const uint8_t* b = s.y + (size_t)y * s.pitch + 4 * mx;
        const Chroma c = yuv_chroma(b[ya::ush422(ORDER) >> 3], b[ya::vsh422(ORDER) >> 3], k);
        uint8_t* o = dst + ((size_t)y * w + 2 * mx) * 3;
        for (int dx = 0; dx < 2; ++dx) store_rgb1(o + 3 * dx, yuv_pixel(b[ya::ysh422(ORDER, dx) >> 3], c, k));
    }
};

// The RGB family (F = the layout: 5 BGR, 6 RGBA, 7 BGRA): row y of the one plane -> row y of the RGB frame, a permutation of bytes;
// alpha is not read.
template <int F>
struct RowsPx {
    static constexpr bool CHROMA_ROWS = false;
    static constexpr int ANY_COLS = 1;
    static constexpr int BPP = F == 5 ? 3 : 4;             // bytes a pixel
    static constexpr int R = F == 6 ? 0 : 2, B = 2 - R;    // where R and B lie in it (G: byte 1)
    __device__ __forceinline__ static Planes dense(const uint8_t* frame, int, int w) { return Planes{frame, nullptr, nullptr, BPP * w, 0}; }
    // 48 / 64 bytes in three / four 16-byte loads
    __device__ __forceinline__ static void wide(const Planes& s, YuvCoef, uint8_t* dst, int, int w, int, int, int y, int x0) {
        if (x0 >= w) return;
        const uint4* in = reinterpret_cast<const uint4*>(s.y + (size_t)y * s.pitch + BPP * x0);
        uint32_t m[4 * BPP];
#pragma unroll
        for (int i = 0; i < BPP; ++i) {
            const uint4 q = in[i];
            m[4 * i] = q.x; m[4 * i + 1] = q.y; m[4 * i + 2] = q.z; m[4 * i + 3] = q.w;
        }
        auto byte_at = [&](int j) { return (m[j >> 2] >> (8 * (j & 3))) & 255u; };
        uint32_t d[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                      // four pixels -> three dwords
            uint32_t px[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int b0 = BPP * (4 * j + i);
                px[i] = byte_at(b0 + R) | (byte_at(b0 + 1) << 8) | (byte_at(b0 + B) << 16);
            }
            pack_rgb4(px, d + 3 * j);
        }
        store_rgb16(dst + ((size_t)y * w + x0) * 3, d);
    }
    // one thread per pixel (column x of row y)
    __device__ __forceinline__ static void any(const Planes& s, YuvCoef, uint8_t* dst, int, int w, int, int, int y, int x) {
        if (x >= w) return;
        const uint8_t* b = s.y + (size_t)y * s.pitch + (size_t)BPP * x;
        uint8_t* o = dst + ((size_t)y * w + x) * 3;
        o[0] = b[R];
        o[1] = b[1];
        o[2] = b[B];
    }
};

// 8-bit raw Bayer (P = the pattern): row y of the RGB frame is the demosaic of row clamp(y, 1, h - 2) of the one plane, column x that
// of column clamp(x, 1, w - 2) (bayer_arith.h).
template <int P>
struct RowsBayer {
    static constexpr bool CHROMA_ROWS = false;
    static constexpr int ANY_COLS = 1;
    __device__ __forceinline__ static Planes dense(const uint8_t* frame, int, int w) { return Planes{frame, nullptr, nullptr, w, 0}; }
    // 16 bytes of each of the three rows around the clamped row in 16-byte loads and the byte on either side of them
    __device__ __forceinline__ static void wide(const Planes& s, YuvCoef, uint8_t* dst, int h, int w, int, int, int y, int x0) {
        if (x0 >= w) return;
        const int cy = ba::tap_pos(y, h), xl = max(x0 - 1, 0), xr = min(x0 + 16, w - 1);
        uint32_t m[3][4], left[3], right[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const uint8_t* row = s.y + (size_t)(cy - 1 + r) * s.pitch;
            const uint4 q = *reinterpret_cast<const uint4*>(row + x0);
            m[r][0] = q.x; m[r][1] = q.y; m[r][2] = q.z; m[r][3] = q.w;
            left[r] = row[xl];
            right[r] = row[xr];
        }
        // column x0 + j of row r of the three, j = -1 .. 16
        auto at = [&](int r, int j) { return j < 0 ? left[r] : j > 15 ? right[r] : (m[r][j >> 2] >> (8 * (j & 3))) & 255u; };
        uint32_t px[16];
#pragma unroll
        for (int j = 0; j < 16; ++j)         // (x0 is even: the column's parity is j's)
            px[j] = ba::demosaic(at(1, j), at(1, j - 1) + at(1, j + 1), at(0, j) + at(2, j),
                                 at(0, j - 1) + at(0, j + 1) + at(2, j - 1) + at(2, j + 1), ba::phase(P, cy, j));
        if (x0 == 0) px[0] = px[1];          // the frame's first and last column: their neighbours'
        if (x0 + 16 == w) px[15] = px[14];
        uint32_t d[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) pack_rgb4(px + 4 * j, d + 3 * j);
        store_rgb16(dst + ((size_t)y * w + x0) * 3, d);
    }
    // one thread per pixel (column x of row y)
    __device__ __forceinline__ static void any(const Planes& s, YuvCoef, uint8_t* dst, int h, int w, int, int, int y, int x) {
        if (x >= w) return;
        const int cy = ba::tap_pos(y, h), cx = ba::tap_pos(x, w);
        const uint8_t *up = s.y + (size_t)(cy - 1) * s.pitch + cx, *mid = up + s.pitch, *dn = mid + s.pitch;
        const uint32_t v = ba::demosaic(mid[0], (uint32_t)mid[-1] + mid[1], (uint32_t)up[0] + dn[0], (uint32_t)up[-1] + up[1] + dn[-1] + dn[1],
                                        ba::phase(P, cy, cx));
        store_rgb1(dst + ((size_t)y * w + x) * 3, v);
    }
};
// What the table bodies below do to a demosaiced pixel (R | G << 8 | B << 16) on its way out: nothing, or the colour stage
// (lt_set_raw_color: matrix, then the output curve in LDS).
struct NoPost { __device__ __forceinline__ uint32_t operator()(uint32_t v) const { return v; } };
struct ColorPost {
    RawColorMat cm;
    const uint8_t* curve;
    __device__ __forceinline__ uint32_t operator()(uint32_t v) const { return ba::color_px(v, cm.m, curve); }
};
// RowsBayer behind a raw table (`lut`: the table in LDS, 1 << bits bytes a row, bits = 8 for bytes): the same two bodies over the conditioned
// mosaic, every site looked up in the table row of its phase before it is summed -- 3 x 18 lookups per 16 pixels (wide), 9 per pixel (any).
// W16: the sites are 16-bit words (pitch in bytes and even), masked to `bits` bits; wide's 16 columns are then 32 bytes, two 16-byte loads a
// row, any's accesses 2 bytes.  LS: behind the lens-shading correction, every site shaded with the gain of its position, read from the gain
// plane `gp` (uint16, w a row), and the pedestal of its phase before it is looked up; the 16 gains of wide's 16 columns are two 16-byte loads
// (w, x0 and the plane's base are multiples of 16).  The bodies differ in how one site (`one`) and the four conditioned dwords of 16 sites
// (`row16`) are obtained, and in nothing else.  A body of its own, so that the plain one above stays the code it was.
// PACK (0 / 1, with W16; -1: none): the rows are MIPI-packed RAW10 / RAW12 (mipi_arith.h), a site two byte accesses, wide's 16 columns 20 / 24
// bytes from a multiple of 4 -- five / six dword loads (every base and pitch of the launch a multiple of 4) -- unpacked into the words of W16.
template <int P, bool W16, bool LS, int PACK = -1>
struct RowsRaw {
    static_assert(PACK < 0 || W16, "packed samples are 10 / 12 bits wide");
    const uint8_t* lut;
    int bits;
    uint32_t mask;                           // (1 << bits) - 1
    const uint16_t* gp;                      // LS
    RawShadeBlack blk;
    __device__ __forceinline__ static Planes dense(const uint8_t* frame, int, int w) {
        if constexpr (PACK >= 0) return Planes{frame, nullptr, nullptr, ma::row_bytes(PACK, w), 0};
        else return Planes{frame, nullptr, nullptr, W16 ? 2 * w : w, 0};
    }
    // the table row of the sites of row parity par_y and column parity par_x
    __device__ __forceinline__ const uint8_t* trow(int par_y, int par_x) const { return lut + ba::lut_row_wide(bits, P, par_y, par_x); }
    __device__ __forceinline__ static uint32_t site(const uint8_t* row, int x) {
        if constexpr (PACK >= 0) return ma::site_at(PACK, row, x);
        else if constexpr (W16) return reinterpret_cast<const uint16_t*>(row)[x];
        else return row[x];
    }
    // site x of the row `row` of the mosaic (row parity py), whose gains are `grow`: (shaded and) looked up
    __device__ __forceinline__ uint32_t one(const uint8_t* row, const uint16_t* grow, int py, int x) const {
        const uint32_t s = site(row, x) & mask;
        if constexpr (LS) {
            const int b = black_of(blk, ba::phase_of(P, py, x & 1));
            return trow(py, x & 1)[sa::shade(s, b, sa::round_term(b), grow[x], (int)mask)];
        } else {
            return trow(py, x & 1)[s];
        }
    }
    // the 16 sites from x0 (even: site 0 of every dword is an even column) of that row -> the four dwords of their conditioned bytes
    __device__ __forceinline__ void row16(const uint8_t* row, const uint16_t* grow, int py, int x0, uint32_t (&m)[4]) const {
        const uint8_t *ta = trow(py, 0), *tb = trow(py, 1);
        sa::Black2 k = {};
        uint32_t g[8] = {};                  // LS: the 16 gains, two a dword
        if constexpr (LS) {
            k = sa::black2(black_of(blk, ba::phase_of(P, py, 0)), black_of(blk, ba::phase_of(P, py, 1)));
            const uint4 ga = *reinterpret_cast<const uint4*>(grow + x0), gb = *reinterpret_cast<const uint4*>(grow + x0 + 8);
            g[0] = ga.x; g[1] = ga.y; g[2] = ga.z; g[3] = ga.w; g[4] = gb.x; g[5] = gb.y; g[6] = gb.z; g[7] = gb.w;
        }
        // four consecutive sites, one dword (bytes) or the two dwords lo, hi (words), whose gains are the two dwords from g[2 j]
        auto four = [&](int j, uint32_t lo, uint32_t hi) {
            if constexpr (W16 && LS) m[j] = sa::shade_condition4w(lo, hi, g[2 * j], g[2 * j + 1], k, ta, tb, mask);
            else if constexpr (W16) m[j] = ba::condition4w(lo, hi, ta, tb, mask);
            else if constexpr (LS) m[j] = sa::shade_condition4(lo, g[2 * j], g[2 * j + 1], k, ta, tb);
            else m[j] = ba::condition4(lo, ta, tb);
        };
        if constexpr (PACK >= 0) {
            constexpr int ND = PACK == ma::PACK10 ? 5 : 6;
            const uint32_t* in = reinterpret_cast<const uint32_t*>(row + ma::first_byte(PACK, x0));
            uint32_t q[ND];
#pragma unroll
            for (int i = 0; i < ND; ++i) q[i] = in[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t lo, hi;
                ma::group4<PACK>(q, j, lo, hi);
                four(j, lo, hi);
            }
        } else if constexpr (W16) {
            const uint4 q0 = *reinterpret_cast<const uint4*>(row + 2 * x0), q1 = *reinterpret_cast<const uint4*>(row + 2 * x0 + 16);
            four(0, q0.x, q0.y); four(1, q0.z, q0.w); four(2, q1.x, q1.y); four(3, q1.z, q1.w);
        } else {
            const uint4 q = *reinterpret_cast<const uint4*>(row + x0);
            four(0, q.x, 0); four(1, q.y, 0); four(2, q.z, 0); four(3, q.w, 0);
        }
    }
    template <class Post>
    __device__ __forceinline__ void wide(const Planes& s, uint8_t* dst, int h, int w, int y, int x0, Post post) const {
        if (x0 >= w) return;
        const int cy = ba::tap_pos(y, h), xl = max(x0 - 1, 0), xr = min(x0 + 16, w - 1);
        uint32_t m[3][4], left[3], right[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const uint8_t* row = s.y + (size_t)(cy - 1 + r) * s.pitch;
            const uint16_t* grow = LS ? gp + (size_t)(cy - 1 + r) * w : nullptr;
            const int py = (cy - 1 + r) & 1;
            row16(row, grow, py, x0, m[r]);
            left[r] = one(row, grow, py, xl);
            right[r] = one(row, grow, py, xr);
        }
        // column x0 + j of row r of the three, j = -1 .. 16
        auto at = [&](int r, int j) { return j < 0 ? left[r] : j > 15 ? right[r] : (m[r][j >> 2] >> (8 * (j & 3))) & 255u; };
        uint32_t px[16];
#pragma unroll
        for (int j = 0; j < 16; ++j)
            px[j] = ba::demosaic(at(1, j), at(1, j - 1) + at(1, j + 1), at(0, j) + at(2, j),
                                 at(0, j - 1) + at(0, j + 1) + at(2, j - 1) + at(2, j + 1), ba::phase(P, cy, j));
        if (x0 == 0) px[0] = px[1];
        if (x0 + 16 == w) px[15] = px[14];
#pragma unroll
        for (int j = 0; j < 16; ++j) px[j] = post(px[j]);
        uint32_t d[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) pack_rgb4(px + 4 * j, d + 3 * j);
        store_rgb16(dst + ((size_t)y * w + x0) * 3, d);
    }
    template <class Post>
    __device__ __forceinline__ void any(const Planes& s, uint8_t* dst, int h, int w, int y, int x, Post post) const {
        if (x >= w) return;
        const int cy = ba::tap_pos(y, h), cx = ba::tap_pos(x, w);
        const uint8_t *up = s.y + (size_t)(cy - 1) * s.pitch, *mid = up + s.pitch, *dn = mid + s.pitch;
        const uint16_t *gu = LS ? gp + (size_t)(cy - 1) * w : nullptr, *gm = LS ? gu + w : nullptr, *gd = LS ? gm + w : nullptr;
        const int py = cy & 1;               // the site's row parity; a neighbour one row away has the other one
        auto u = [&](int i) { return one(up, gu, py ^ 1, cx + i); };
        auto m = [&](int i) { return one(mid, gm, py, cx + i); };
        auto d = [&](int i) { return one(dn, gd, py ^ 1, cx + i); };
        const uint32_t v = ba::demosaic(m(0), m(-1) + m(1), u(0) + d(0), u(-1) + u(1) + d(-1) + d(1), ba::phase(P, cy, cx));
        store_rgb1(dst + ((size_t)y * w + x) * 3, post(v));
    }
};
// the description of a layout (none for 0, plain RGB: its rows are shown as they are)
template <int L>
using RowsOf = std::conditional_t<L <= 2, Rows420<L>, std::conditional_t<L <= 4, Rows422<L - 3>, std::conditional_t<L <= 7, RowsPx<L>, RowsBayer<L - 16>>>>;

// Entries into the surface table, as a kernel argument (no host memory has to outlive the call): entry i -> tab[first + i].
__global__ __launch_bounds__(64) void k_write_surf_entries(SurfEntry* __restrict__ tab, int first, int n, SurfChunk ch) {
    const int i = (int)threadIdx.x;
    if (i >= n) return;
    const SurfEntry e = ch.e[i];
    tab[first + i] = e;
}

// The one entry point: layout x source x body.  Frame blockIdx.z of the launch is the slot's dense staging frame at src.p + blockIdx.z *
// src.stride, or (SURF) the surface of entry blockIdx.z of the chunk, which travels as the kernel argument; launch row blockIdx.y
// counts from r0 (CHROMA_ROWS: from chroma row r0 / 2).  (What every layout reads comes first in the parameter list, so that a form that
// reads nothing else fetches its arguments in one piece.)
struct DenseFrames { const uint8_t* p; size_t stride; };
template <int LAYOUT, bool SURF, bool WIDE>
__global__ __launch_bounds__(256) void k_rows_to_rgb(std::conditional_t<SURF, SurfChunk, DenseFrames> src, uint8_t* __restrict__ rgb,
                                                    size_t rgb_stride, int w, int r0, int r1, int h, YuvCoef k) {
    typedef RowsOf<LAYOUT> D;
    Planes p;
    if constexpr (SURF) p = surf_planes(src.e[blockIdx.z]);
    else p = D::dense(src.p + (size_t)blockIdx.z * src.stride, h, w);
    uint8_t* dst = rgb + (size_t)blockIdx.z * rgb_stride;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), row = (D::CHROMA_ROWS ? r0 >> 1 : r0) + (int)blockIdx.y;
    if constexpr (WIDE) D::wide(p, k, dst, h, w, r0, r1, row, i * 16);
    else D::any(p, k, dst, h, w, r0, r1, row, i);
}

// The raw Bayer row conversion behind a raw table: RowsRaw's bodies in k_rows_to_rgb's two launch shapes (64 threads for the wide body, 256
// for the byte-wise one), STAGES and `r` as k_raw_walk_rows takes them.  The table, and the curve in front of it, are staged in 16-byte
// pieces by the whole workgroup before any thread leaves: static LDS for 8-bit samples, the launch's dynamic LDS for 16-bit ones.  Launched
// in k_rows_to_rgb's place whenever there is a table.
// (the body: shared by the kernels that are given `r` and by those that find it in their frame's raw set, k_rawset_rows_rgb / k_packset_rows_rgb)
template <int PATTERN, bool SURF, bool WIDE, int STAGES, int PACK>
__device__ __forceinline__ void raw_rows(uint8_t* lds, const std::conditional_t<SURF, SurfChunk, DenseFrames>& src, uint8_t* __restrict__ rgb,
                                         size_t rgb_stride, int w, int r0, int h, const RawStages& r) {
    constexpr bool W16 = (STAGES & 1) != 0, CC = (STAGES & 2) != 0, LS = (STAGES & 4) != 0;
    constexpr int THREADS = WIDE ? 64 : 256, CURVE = CC ? 256 : 0;
    const int bits = W16 ? r.bits : 8;
    for (int i = threadIdx.x; i < CURVE / 16 + (1 << (bits - 2)); i += THREADS) reinterpret_cast<uint4*>(lds)[i] = reinterpret_cast<const uint4*>(r.table)[i];
    __syncthreads();
    typedef RowsRaw<PATTERN, W16, LS, PACK> D;
    const D body{lds + CURVE, bits, (1u << bits) - 1u, r.gains, r.blk};
    Planes p;
    if constexpr (SURF) p = surf_planes(src.e[blockIdx.z]);
    else p = D::dense(src.p + (size_t)blockIdx.z * src.stride, h, w);
    uint8_t* dst = rgb + (size_t)blockIdx.z * rgb_stride;
    const int i = (int)(blockIdx.x * THREADS + threadIdx.x), row = r0 + (int)blockIdx.y;
    std::conditional_t<CC, ColorPost, NoPost> post{};
    if constexpr (CC) post = ColorPost{r.cm, lds};
    if constexpr (WIDE) body.wide(p, dst, h, w, row, i * 16, post);
    else body.any(p, dst, h, w, row, i, post);
}
template <int PATTERN, bool SURF, bool WIDE, int STAGES>
__global__ __launch_bounds__(256) void k_raw_rows_rgb(std::conditional_t<SURF, SurfChunk, DenseFrames> src, uint8_t* __restrict__ rgb,
                                                     size_t rgb_stride, int w, int r0, int h, RawStages r) {
    constexpr bool W16 = (STAGES & 1) != 0, CC = (STAGES & 2) != 0;
    raw_rows<PATTERN, SURF, WIDE, STAGES, -1>(raw_lds<W16, CC ? 256 : 0>(), src, rgb, rgb_stride, w, r0, h, r);
}

// ... over MIPI-packed RAW10 / RAW12 rows (PACK): k_raw_rows_rgb's 16-bit forms, RowsRaw's two bodies with the packed accesses.  The wide body
// needs every base and pitch of the frames a multiple of 4 only (and those of the RGB frames a multiple of 16, as ever).
template <int PATTERN, bool SURF, bool WIDE, int STAGES, int PACK>
__global__ __launch_bounds__(256) void k_mipi_rows_rgb(std::conditional_t<SURF, SurfChunk, DenseFrames> src, uint8_t* __restrict__ rgb,
                                                      size_t rgb_stride, int w, int r0, int h, RawStages r) {
    static_assert((STAGES & 1) != 0, "packed samples are 10 / 12 bits wide: behind the wide table");
    raw_rows<PATTERN, SURF, WIDE, STAGES, PACK>(s_lut_wide, src, rgb, rgb_stride, w, r0, h, r);
}

// The set-per-slot forms of the two row conversions above: frame blockIdx.z of the launch is conditioned with its slot's raw set -- id byte
// blockIdx.z of `rids`, entry rsets[id], by scalar loads, as in k_rawset_walk_rows -- and the workgroup stages that set's table.
template <int PATTERN, bool SURF, bool WIDE, int STAGES>
__global__ __launch_bounds__(256) void k_rawset_rows_rgb(std::conditional_t<SURF, SurfChunk, DenseFrames> src, uint8_t* __restrict__ rgb,
                                                        size_t rgb_stride, int w, int r0, int h, const RawSetEntry* __restrict__ rsets, CalIds rids, int bits) {
    constexpr bool W16 = (STAGES & 1) != 0, CC = (STAGES & 2) != 0;
    raw_rows<PATTERN, SURF, WIDE, STAGES, -1>(raw_lds<W16, CC ? 256 : 0>(), src, rgb, rgb_stride, w, r0, h, stages_of_set(rsets, rids, (int)blockIdx.z, bits));
}
template <int PATTERN, bool SURF, bool WIDE, int STAGES, int PACK>
__global__ __launch_bounds__(256) void k_packset_rows_rgb(std::conditional_t<SURF, SurfChunk, DenseFrames> src, uint8_t* __restrict__ rgb,
                                                         size_t rgb_stride, int w, int r0, int h, const RawSetEntry* __restrict__ rsets, CalIds rids, int bits) {
    static_assert((STAGES & 1) != 0, "packed samples are 10 / 12 bits wide: behind the wide table");
    raw_rows<PATTERN, SURF, WIDE, STAGES, PACK>(s_lut_wide, src, rgb, rgb_stride, w, r0, h, stages_of_set(rsets, rids, (int)blockIdx.z, bits));
}

// Rows [r0, r1) of RGB surfaces -> the same rows of the slots' camera frames (row_bytes = 3 w, dense): a pitched row copy, one
// thread per 16 bytes (WIDE: every base and pitch of the launch a multiple of 16) or per byte.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_surf_copy_rows(SurfChunk ch, uint8_t* __restrict__ rgb, size_t rgb_stride, int row_bytes, int r0) {
    constexpr int V = WIDE ? 16 : 1;
    const int xb = (int)(blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (xb >= row_bytes) return;
    const int y = r0 + (int)blockIdx.y;
    const SurfEntry& e = ch.e[blockIdx.z];
    const uint8_t* src = reinterpret_cast<const uint8_t*>(e.plane[0]) + (size_t)y * e.pitch + xb;
    uint8_t* dst = rgb + (size_t)blockIdx.z * rgb_stride + (size_t)y * row_bytes + xb;
    if constexpr (WIDE) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    else *dst = *src;
}

struct LabLut {
    const uint16_t* gamma_tab;
    const uint16_t* cbrt_tab;
};

__device__ __forceinline__ int lab_b_of(int r, int g, int b, const uint16_t* gt, const uint16_t* ct,
                                        const int32_t* C) {
    const int R = gt[r], G = gt[g], B = gt[b];
    int iy = (__mul24(R, C[3]) + __mul24(G, C[4]) + __mul24(B, C[5]) + (1 << 11)) >> 12;   // R,G,B <= 2040, C < 4096
    int iz = (__mul24(R, C[6]) + __mul24(G, C[7]) + __mul24(B, C[8]) + (1 << 11)) >> 12;
    iy = iy > 3071 ? 3071 : iy;
    iz = iz > 3071 ? 3071 : iz;
    const int fY = ct[iy], fZ = ct[iz];
    const int v = (__mul24(200, fY - fZ) + 128 * (1 << 15) + (1 << 14)) >> 15;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ void stage_lab_tables(uint16_t* s_gamma, uint16_t* s_cbrt, int32_t* s_coef,
                                                 const uint16_t* gamma_tab, const uint16_t* cbrt_tab,
                                                 const int32_t* coeffs) {
    // 16 bytes per load where the tables allow it (the context's are hipMalloc'ed): 2 loads per thread instead of 13 -- a block
    // of k_warp_split4 walks a few slot pairs only, and these loads were a third of its vector-memory instructions
    if (((reinterpret_cast<uintptr_t>(gamma_tab) | reinterpret_cast<uintptr_t>(cbrt_tab)) & 15u) == 0) {
        for (int i = threadIdx.x; i < 256 / 8; i += blockDim.x) reinterpret_cast<uint4*>(s_gamma)[i] = reinterpret_cast<const uint4*>(gamma_tab)[i];
        for (int i = threadIdx.x; i < 3072 / 8; i += blockDim.x) reinterpret_cast<uint4*>(s_cbrt)[i] = reinterpret_cast<const uint4*>(cbrt_tab)[i];
    } else {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) s_gamma[i] = gamma_tab[i];
        for (int i = threadIdx.x; i < 3072; i += blockDim.x) s_cbrt[i] = cbrt_tab[i];
    }
    if (threadIdx.x < 9) s_coef[threadIdx.x] = coeffs[threadIdx.x];
    __syncthreads();
}

// exact 8-bit remap blend of the three channels of four RGBX taps:
//   sum_i w_i p_i with w = {(32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx fy} * 32, then (s + 2^14) >> 15,
// which equals ((32-fy) h0 + fy h1 + 512) >> 10 with h = (32-fx) p_left + fx p_right  (same integers).
__device__ __forceinline__ void blend_taps(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11, int fx, int fy,
                                           int (&rgb)[3]) {
    const int gx = 32 - fx, gy = 32 - fy;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int h0 = __mul24((int)((t00 >> (8 * ch)) & 255u), gx) + __mul24((int)((t01 >> (8 * ch)) & 255u), fx);
        const int h1 = __mul24((int)((t10 >> (8 * ch)) & 255u), gx) + __mul24((int)((t11 >> (8 * ch)) & 255u), fx);
        rgb[ch] = (__mul24(h0, gy) + __mul24(h1, fy) + 512) >> 10;
    }
}

__device__ __forceinline__ void warp_pixel(const uint32_t* __restrict__ src, const FrontEndGeom& g, int sx, int sy,
                                           int f, const uint16_t* gt, const uint16_t* ct, const int32_t* C, int& r_out,
                                           int& b_out) {
    const int fx = f & 31, fy = f >> 5;
    // taps outside the camera frame are 0; in-frame taps always fall inside rows [r0, r0+nrows)
    const int ry0 = sy - g.r0, ry1 = sy + 1 - g.r0;
    const bool y0 = sy >= 0 && sy < g.img_h && ry0 >= 0 && ry0 < g.nrows;
    const bool y1 = sy + 1 >= 0 && sy + 1 < g.img_h && ry1 >= 0 && ry1 < g.nrows;
    const bool x0 = sx >= 0 && sx < g.img_w, x1 = sx + 1 >= 0 && sx + 1 < g.img_w;
    const int cy0 = min(max(ry0, 0), g.nrows - 1), cy1 = min(max(ry1, 0), g.nrows - 1);
    const int cx0 = min(max(sx, 0), g.img_w - 1), cx1 = min(max(sx + 1, 0), g.img_w - 1);
    const int o0 = __mul24(cy0, g.img_w), o1 = __mul24(cy1, g.img_w);
    uint32_t t00 = src[2 * (o0 + cx0)], t01 = src[2 * (o0 + cx1)];   // pixels of one slot are two dwords apart
    uint32_t t10 = src[2 * (o1 + cx0)], t11 = src[2 * (o1 + cx1)];
    t00 = (y0 && x0) ? t00 : 0u;
    t01 = (y0 && x1) ? t01 : 0u;
    t10 = (y1 && x0) ? t10 : 0u;
    t11 = (y1 && x1) ? t11 : 0u;
    int rgb[3];
    blend_taps(t00, t01, t10, t11, fx, fy, rgb);
    r_out = rgb[0];
    b_out = lab_b_of(rgb[0], rgb[1], rgb[2], gt, ct, C);
}

// Four adjacent bird's-eye pixels per thread: bilinear samples of the RGBX undistorted rows, then
// one dword store to the R plane and one to the Lab-b plane.  `quads` = pixels / 4 (w % 4 == 0).
// The remap table entry of a quad is the same for every frame, so a thread keeps it (and the tap
// offsets derived from it) in registers and walks `ppb` consecutive slot PAIRS with it: the two taps of a row are one
// 16-byte load {left.even, left.odd, right.even, right.odd} that serves both slots of the pair.
// Slots [first_slot, first_slot + n); `und` is the base of the whole buffer, planeR / planeB point at first_slot's planes.

// Latency is hidden by occupancy, not by prefetch: with the taps of the next slot pair in flight (two sets of 8 x 16 bytes)
// the kernel needs 97 VGPRs = 4 waves per SIMD; with one set it fits 64 = 8 waves and runs 6 % faster alone and 3 % faster
// end to end, where it shares the CUs with the other slices' kernels (-DLT_WARP_PREFETCH=1 -DLT_WARP_WAVES=5 for the A/B).
#ifndef LT_WARP_PREFETCH
#define LT_WARP_PREFETCH 0
#endif
#ifndef LT_WARP_WAVES
#define LT_WARP_WAVES 8
#endif
// LAB_CLAMP: the cube-root table index keeps its clamp to 3071 (false where launch_warp_split's caller has shown it dead for the
// tables of this context: front_arith.h, lab_clamp_is_dead).
#ifndef LT_WARP_F32
#define LT_WARP_F32 0   // the blend as an fp32 fma chain (front_arith.h; exact): measured 0.733 ms against 0.540 -- the byte -> float conversions are 4-cycle instructions and the packed fma form spills; kept for the A/B
#endif
template <bool LAB_CLAMP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LT_WARP_WAVES, LT_WARP_WAVES))) void k_warp_split4(const uint32_t* __restrict__ und, size_t und_px, int first_slot,
                                                    const int16_t* __restrict__ wxy,
                                                    const uint16_t* __restrict__ wfrac, FrontEndGeom g,
                                                    const uint16_t* __restrict__ gamma_tab,
                                                    const uint16_t* __restrict__ cbrt_tab,
                                                    const int32_t* __restrict__ coeffs, uint8_t* __restrict__ planeR,
                                                    uint8_t* __restrict__ planeB, size_t plane_stride, int n, int ppb,
                                                    int remap) {
    __shared__ alignas(16) uint16_t s_gamma[256];
    __shared__ alignas(16) uint16_t s_cbrt[3072];
    __shared__ int32_t s_coef[9];
    // gamma LUT and the Y / Z rows of the matrix folded into one table per channel: s_yz[ch][v] = gamma[v] * (C[3+ch], C[6+ch]),
    // the rounding constant of DESCALE(., 12) added to the red entries -- one 8-byte LDS read per channel replaces a 16-bit
    // read, two multiplies / multiply-adds and the rounding add (the kernel is at 80 % of the VALU issue ceiling)
    __shared__ fa::YZ s_yz[3][256];
    const size_t quads = ((size_t)g.warp_h * g.warp_w) >> 2;
    const uint32_t id = xcd_block(blockIdx.z * gridDim.x + blockIdx.x, gridDim.x * gridDim.z, remap);
    const uint32_t bz = id / gridDim.x, bx = id - bz * gridDim.x;
    const size_t qi = (size_t)bx * blockDim.x + threadIdx.x;
    const size_t qc = qi < quads ? qi : quads - 1;
    // the table entry is requested before the Lab tables are staged: both latencies overlap
    const uint4 xy = reinterpret_cast<const uint4*>(wxy)[qc];        // 4 x (sx, sy) int16 pairs
    const uint2 fr = reinterpret_cast<const uint2*>(wfrac)[qc];      // 4 x u16
    {
        const int v = threadIdx.x;   // 256 threads: one table row each
        const uint32_t gv = gamma_tab[v];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            s_yz[ch][v] = fa::yz_row(gv, coeffs, ch);
    }
    stage_lab_tables(s_gamma, s_cbrt, s_coef, gamma_tab, cbrt_tab, coeffs);
    if (qi >= quads) return;
    // this walk: pairs [pa, pb) of the buffer, i.e. slots [2 pa, 2 pb) clipped to [first_slot, first_slot + n)
    const int pair_lo = first_slot >> 1, pair_hi = (first_slot + n + 1) >> 1;
    const int pa = pair_lo + (int)bz * ppb, pb = min(pa + ppb, pair_hi);
    const int s_lo = max(2 * pa, first_slot), s_hi = min(2 * pb, first_slot + n);   // slots this walk writes
    if (s_hi <= s_lo) return;
    uint8_t* const outR = planeR + (size_t)(s_lo - first_slot) * plane_stride;
    uint8_t* const outB = planeB + (size_t)(s_lo - first_slot) * plane_stride;
    const uint32_t xyv[4] = {xy.x, xy.y, xy.z, xy.w};
    const uint32_t frv[4] = {fr.x & 0xffffu, fr.x >> 16, fr.y & 0xffffu, fr.y >> 16};
    // 87 % of the bird's-eye view samples strictly inside the staged rows: skip every border test there
    bool inside = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int sx = (int16_t)(xyv[i] & 0xffffu), sy = (int16_t)(xyv[i] >> 16);
        inside = inside && sx >= 0 && sx + 1 < g.img_w && sy >= g.r0 && sy + 1 < g.r0 + g.nrows && sy + 1 < g.img_h;
    }
    if (inside) {
        // The four tap weights of a pixel (products of the 5-bit fractions) are frame-independent: floats, scaled so that the
        // blend is an fma chain of the 2-cycle class that ends in 8 x the value (front_arith.h; exact, the same integer as
        // (sum_i w_i p_i + 2^9) >> 10).
#if LT_WARP_F32
        fa::Weights wt[4];
#else
        fa::WeightsI wt[4];
#endif
        int toff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int sx = (int16_t)(xyv[i] & 0xffffu), sy = (int16_t)(xyv[i] >> 16);
            toff[i] = (__mul24(sy - g.r0, g.img_w) + sx) * 8;            // byte offset of the left tap inside a pair
#if LT_WARP_F32
            wt[i] = fa::weights8((int)(frv[i] & 31u), (int)(frv[i] >> 5));
#else
            wt[i] = fa::weights_i((int)(frv[i] & 31u), (int)(frv[i] >> 5));
#endif
        }
        // Taps and outputs go through buffer descriptors of this walk: descriptor + 32-bit lane offset + scalar
        // pair / frame offset, so no access pays a 64-bit VALU address add.
        constexpr int RSRC_RAW = 0x00027000;   // untyped 32-bit buffer, no swizzle
        const int pair_b = (int)(und_px * 8);
        const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(und + (size_t)pa * 2 * und_px), 0, (pb - pa) * pair_b, RSRC_RAW);
        const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc(outR, 0, (s_hi - s_lo) * (int)plane_stride, RSRC_RAW);
        const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(outB, 0, (s_hi - s_lo) * (int)plane_stride, RSRC_RAW);
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const int row_b = g.img_w * 8, out_off = (int)qi * 4;
        u32x4 tapA[8], tapB[8];   // [0..3] top row, [4..7] bottom row of the four pixels; A / B alternate between pairs
        auto fetch = [&](u32x4 (&t)[8], int p) __attribute__((always_inline)) {
            const int po = (min(p, pb - 1) - pa) * pair_b;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                t[i] = __builtin_amdgcn_raw_buffer_load_b128(urs, toff[i], po, 0);
                t[4 + i] = __builtin_amdgcn_raw_buffer_load_b128(urs, toff[i] + row_b, po, 0);
            }
        };
        auto blend_pair = [&](const u32x4 (&t)[8], int p) __attribute__((always_inline)) {
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const int slot = 2 * p + f;
                if (slot < s_lo || slot >= s_hi) continue;     // wave-uniform: the odd slot in front of / behind the range
                uint32_t oR = 0, oB = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t ta = t[i][f], tb = t[i][2 + f], ba = t[4 + i][f], bb = t[4 + i][2 + f];
#if !LT_WARP_F32
                    // The packed weights stay packed across the loop (8 registers, not 16: with 16 the kernel kept two values in
                    // scratch and reloaded them for every slot pair, through the memory pipe it is co-bound by): opaque here, so
                    // the halves are selected inside the loop, by the multiply's own operand select.
                    fa::WeightsI wq = wt[i];
                    asm volatile("" : "+v"(wq.top), "+v"(wq.bot));
#else
                    const fa::Weights wq = wt[i];
#endif
                    // 8 x the blended channel = the byte offset of its row in s_yz[ch]: no shift between blend and table
                    uint32_t r8 = fa::blend8<0>(ta, tb, ba, bb, wq) & fa::ROW8_MASK;
                    const uint32_t g8 = fa::blend8<1>(ta, tb, ba, bb, wq) & fa::ROW8_MASK;
                    const uint32_t b8 = fa::blend8<2>(ta, tb, ba, bb, wq) & fa::ROW8_MASK;
                    auto row = [&](int ch, uint32_t off) __attribute__((always_inline)) {
                        return *reinterpret_cast<const fa::YZ*>(reinterpret_cast<const char*>(s_yz[ch]) + off);
                    };
                    int b = fa::lab_b_rows<LAB_CLAMP>(row(0, r8), row(1, g8), row(2, b8), s_cbrt);
                    // Opaque to the optimiser on purpose: with the value ranges visible, hipcc (ROCm 7.2) folded the
                    // four byte inserts into a 16-bit combine that leaked bits 16+ of an unshifted Lab value into the
                    // third pixel (caught by the parity test); the barrier costs nothing at run time.
#ifndef LT_CASE_WARP_NO_BARRIER   // tools/toolchain_cases.sh builds the kernel without it to check whether the case still exists
                    asm volatile("" : "+v"(r8), "+v"(b));
#endif
                    oR |= i == 0 ? r8 >> 3 : r8 << (8 * i - 3);      // r8 = 8 x red, bits 3..10
                    oB |= ((uint32_t)b & 255u) << (8 * i);
                }
                __builtin_amdgcn_raw_buffer_store_b32(oR, rrs, out_off, (slot - s_lo) * (int)plane_stride, 0);
                __builtin_amdgcn_raw_buffer_store_b32(oB, brs, out_off, (slot - s_lo) * (int)plane_stride, 0);
            }
        };
        // two pairs per trip, the tap registers alternate: the taps of the next pair are in flight while this one is
        // blended, and nothing is copied at the back edge
#if LT_WARP_PREFETCH
        fetch(tapA, pa);
        for (int p = pa; p < pb; p += 2) {
            fetch(tapB, p + 1);
            blend_pair(tapA, p);
            if (p + 1 >= pb) break;
            fetch(tapA, p + 2);
            blend_pair(tapB, p + 1);
        }
#else
        for (int p = pa; p < pb; ++p) {
            fetch(tapA, p);
            blend_pair(tapA, p);
        }
        (void)tapB;
#endif
        return;
    }
    // 13 % of the bird's-eye view (the bottom corner triangles) samples entirely outside the camera frame: every tap
    // is the constant border 0, so R = 0 and Lab-b = b(0,0,0) for every frame -- no loads, no blend.
    bool none = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int sx = (int16_t)(xyv[i] & 0xffffu), sy = (int16_t)(xyv[i] >> 16), ry0 = sy - g.r0, ry1 = ry0 + 1;
        const bool y0 = sy >= 0 && sy < g.img_h && ry0 >= 0 && ry0 < g.nrows;
        const bool y1 = sy + 1 >= 0 && sy + 1 < g.img_h && ry1 >= 0 && ry1 < g.nrows;
        const bool x0 = sx >= 0 && sx < g.img_w, x1 = sx + 1 >= 0 && sx + 1 < g.img_w;
        none = none && !((y0 || y1) && (x0 || x1));
    }
    if (none) {
        const uint32_t oB = (uint32_t)lab_b_of(0, 0, 0, s_gamma, s_cbrt, s_coef) * 0x01010101u;
        for (int slot = s_lo; slot < s_hi; ++slot) {
            reinterpret_cast<uint32_t*>(outR + (size_t)(slot - s_lo) * plane_stride)[qi] = 0u;
            reinterpret_cast<uint32_t*>(outB + (size_t)(slot - s_lo) * plane_stride)[qi] = oB;
        }
        return;
    }
    for (int slot = s_lo; slot < s_hi; ++slot) {
        const uint32_t* src = und + und_slot_base(und_px, slot);
        uint32_t oR = 0, oB = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int sx = (int16_t)(xyv[i] & 0xffffu), sy = (int16_t)(xyv[i] >> 16);
            int r, b;
            warp_pixel(src, g, sx, sy, (int)frv[i], s_gamma, s_cbrt, s_coef, r, b);
            asm volatile("" : "+v"(r), "+v"(b));
            oR |= ((uint32_t)r & 255u) << (8 * i);
            oB |= ((uint32_t)b & 255u) << (8 * i);
        }
        reinterpret_cast<uint32_t*>(outR + (size_t)(slot - s_lo) * plane_stride)[qi] = oR;
        reinterpret_cast<uint32_t*>(outB + (size_t)(slot - s_lo) * plane_stride)[qi] = oB;
    }
}

// any width: one pixel per thread
__global__ __launch_bounds__(256) void k_warp_split1(const uint32_t* __restrict__ und, size_t und_px, int first_slot,
                                                    const int16_t* __restrict__ wxy,
                                                    const uint16_t* __restrict__ wfrac, FrontEndGeom g,
                                                    const uint16_t* __restrict__ gamma_tab,
                                                    const uint16_t* __restrict__ cbrt_tab,
                                                    const int32_t* __restrict__ coeffs, uint8_t* __restrict__ planeR,
                                                    uint8_t* __restrict__ planeB, size_t plane_stride) {
    __shared__ alignas(16) uint16_t s_gamma[256];
    __shared__ alignas(16) uint16_t s_cbrt[3072];
    __shared__ int32_t s_coef[9];
    stage_lab_tables(s_gamma, s_cbrt, s_coef, gamma_tab, cbrt_tab, coeffs);
    const size_t npix = (size_t)g.warp_h * g.warp_w;
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= npix) return;
    int r, b;
    warp_pixel(und + und_slot_base(und_px, first_slot + (int)blockIdx.z), g, wxy[o * 2], wxy[o * 2 + 1], wfrac[o], s_gamma, s_cbrt,
               s_coef, r, b);
    planeR[(size_t)blockIdx.z * plane_stride + o] = (uint8_t)r;
    planeB[(size_t)blockIdx.z * plane_stride + o] = (uint8_t)b;
}

// The table-per-slot form of the warp: PX adjacent bird's-eye pixels of ONE slot per thread (4 where the width is a multiple of 4:
// one dword store per plane; else 1), the table entry from the slot's calibration set (SlotTables: scalar loads, the slot is
// blockIdx.z).  Slots 2p and 2p + 1 may belong to different sets, so nothing here is shared between the partners of a pair: every
// tap is the slot's own dword of the pair-interleaved rows (warp_pixel over und_slot_base), blended and split by warp_pixel with
// the staged Lab tables, as k_warp_split1 and the border path of k_warp_split4 do.
template <int PX>
__global__ __launch_bounds__(256) void k_warp_cal(const uint32_t* __restrict__ und, size_t und_px, int first_slot,
                                                 const CalTables* __restrict__ sets, CalIds ids, FrontEndGeom g,
                                                 const uint16_t* __restrict__ gamma_tab, const uint16_t* __restrict__ cbrt_tab,
                                                 const int32_t* __restrict__ coeffs, uint8_t* __restrict__ planeR,
                                                 uint8_t* __restrict__ planeB, size_t plane_stride) {
    __shared__ alignas(16) uint16_t s_gamma[256];
    __shared__ alignas(16) uint16_t s_cbrt[3072];
    __shared__ int32_t s_coef[9];
    const int z = (int)blockIdx.z;
    const CalTables& t = SlotTables{sets, &ids}.of(z);
    const int16_t* wxy = t.wxy;
    const uint16_t* wfrac = t.wfrac;
    const size_t units = ((size_t)g.warp_h * g.warp_w) / PX;
    const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t uc = u < units ? u : units - 1;
    uint32_t xyv[PX], frv[PX];
    // the table entry is requested before the Lab tables are staged: both latencies overlap
    if constexpr (PX == 4) {
        const uint4 xy = reinterpret_cast<const uint4*>(wxy)[uc];        // 4 x (sx, sy) int16 pairs
        const uint2 fr = reinterpret_cast<const uint2*>(wfrac)[uc];      // 4 x u16
        xyv[0] = xy.x, xyv[1] = xy.y, xyv[2] = xy.z, xyv[3] = xy.w;
        frv[0] = fr.x & 0xffffu, frv[1] = fr.x >> 16, frv[2] = fr.y & 0xffffu, frv[3] = fr.y >> 16;
    } else {
        xyv[0] = reinterpret_cast<const uint32_t*>(wxy)[uc];
        frv[0] = wfrac[uc];
    }
    stage_lab_tables(s_gamma, s_cbrt, s_coef, gamma_tab, cbrt_tab, coeffs);
    if (u >= units) return;
    const uint32_t* src = und + und_slot_base(und_px, first_slot + z);
    uint32_t oR = 0, oB = 0;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        const int sx = (int16_t)(xyv[i] & 0xffffu), sy = (int16_t)(xyv[i] >> 16);
        int r, b;
        warp_pixel(src, g, sx, sy, (int)frv[i], s_gamma, s_cbrt, s_coef, r, b);
        asm volatile("" : "+v"(r), "+v"(b));     // (the byte inserts stay byte inserts: the note in k_warp_split4)
        oR |= ((uint32_t)r & 255u) << (8 * i);
        oB |= ((uint32_t)b & 255u) << (8 * i);
    }
    if constexpr (PX == 4) {
        reinterpret_cast<uint32_t*>(planeR + (size_t)z * plane_stride)[u] = oR;
        reinterpret_cast<uint32_t*>(planeB + (size_t)z * plane_stride)[u] = oB;
    } else {
        planeR[(size_t)z * plane_stride + u] = (uint8_t)oR;
        planeB[(size_t)z * plane_stride + u] = (uint8_t)oB;
    }
}

// filter_lane_points() entry on an already-warped RGB image (lane_tracker.py:207-208)
__global__ __launch_bounds__(256) void k_split_bev(const uint8_t* __restrict__ bev, size_t bev_stride, int npix,
                                                  const uint16_t* __restrict__ gamma_tab,
                                                  const uint16_t* __restrict__ cbrt_tab,
                                                  const int32_t* __restrict__ coeffs, uint8_t* __restrict__ planeR,
                                                  uint8_t* __restrict__ planeB, size_t plane_stride) {
    __shared__ alignas(16) uint16_t s_gamma[256];
    __shared__ alignas(16) uint16_t s_cbrt[3072];
    __shared__ int32_t s_coef[9];
    stage_lab_tables(s_gamma, s_cbrt, s_coef, gamma_tab, cbrt_tab, coeffs);
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (size_t)npix) return;
    const uint8_t* p = bev + (size_t)blockIdx.z * bev_stride + o * 3;
    const int r = p[0], gg = p[1], b = p[2];
    planeR[(size_t)blockIdx.z * plane_stride + o] = (uint8_t)r;
    planeB[(size_t)blockIdx.z * plane_stride + o] = (uint8_t)lab_b_of(r, gg, b, s_gamma, s_cbrt, s_coef);
}

__global__ __launch_bounds__(256) void k_undistorted_to_rgb(const uint32_t* __restrict__ und, size_t und_px, int first_slot,
                                                           int nrows, int w, uint8_t* __restrict__ out) {
    const size_t plane = (size_t)nrows * w;
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= plane) return;
    const uint32_t v = und[und_slot_base(und_px, first_slot + (int)blockIdx.z) + 2 * o];
    uint8_t* dst = out + (size_t)blockIdx.z * plane * 3 + o * 3;
    dst[0] = (uint8_t)v;
    dst[1] = (uint8_t)(v >> 8);
    dst[2] = (uint8_t)(v >> 16);
}

}  // namespace

// Frames one thread walks with its remap-table entry: as many as possible (the table read, the tap address
// arithmetic and one memory round trip are paid once per walk) while the launch still has a few groups of
// frames, so that small batches keep their parallelism.
static int xcd_remap() {
    static const int v = [] { const char* e = LT_EXP_ENV("LT_XCD_REMAP"); return e ? std::atoi(e) : 1; }();
    return v;
}

static int frames_per_thread(int n) {
    static const int cap = [] { const char* e = LT_EXP_ENV("LT_FRONTEND_FPB"); int v = e ? std::atoi(e) : 16; return v < 1 ? 1 : v; }();
    int fpb = n / 8;
    return fpb < 1 ? 1 : (fpb > cap ? cap : fpb);
}

// layout -> f(std::integral_constant<int, layout>{}): the one place where the host turns the number into a template argument
template <class F>
static void with_layout(int layout, F&& f) {
    switch (layout) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 17: return f(std::integral_constant<int, 17>{});
        case 18: return f(std::integral_constant<int, 18>{});
        case 19: return f(std::integral_constant<int, 19>{});
    }
}

// the pattern of a raw Bayer layout (its low two bits) -> f(std::integral_constant<int, pattern>{}), for the raw kernels
template <class F>
static void with_pattern(int layout, F&& f) {
    switch (layout & 3) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
    }
}
// ... and what runs around their demosaic -> f(std::integral_constant<int, STAGES>{}): bit 0 16-bit samples, bit 1 the colour stage, bit 2 the
// shading map
template <class F>
static void with_stages(const RawStages& raw, F&& f) {
    switch ((raw.bits > 8 ? 1 : 0) | (raw.color ? 2 : 0) | (raw.gains ? 4 : 0)) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
    }
}
// the dynamic LDS of a raw kernel: the wide table, behind the curve where there is a colour stage (8-bit samples: static LDS)
static size_t raw_dynamic_lds(const RawStages& raw) { return raw.bits > 8 ? ((size_t)4 << raw.bits) + (raw.color ? 256 : 0) : 0; }

static CalIds pack_ids(const uint8_t* ids, int m) {
    CalIds c{};
    for (int i = 0; i < m; ++i) c.w[i >> 2] |= (uint32_t)ids[i] << (8 * (i & 3));
    return c;
}

// One launch of the walk over the n frames of `src`: behind a raw table the raw walk, else the walk of the layout.  Plain RGB frames of the
// slots that are not dword-aligned, dword-strided and below 2^30 bytes (a larger frame: 64-bit addresses) -- or all of them, any_byte --
// take the form that fetches at any byte.
template <bool PER_SLOT>
static void launch_walk(hipStream_t s, dim3 grid, FrameSource src, int layout, YuvCoef k, const int16_t* uxy, const uint16_t* ufrac,
                        const CalTables* sets, const CalIds& ids, FrontEndGeom g, uint32_t* und, size_t und_px, int first_slot, int n, int fpb,
                        bool any_byte, const RawStages& raw, const RawSetEntry* rsets = nullptr, const CalIds& rids = CalIds{}) {
    const bool aligned = !any_byte && ((uintptr_t)src.frames & 3) == 0 && (src.stride & 3) == 0 && src.stride < (1u << 30);
    const int remap = xcd_remap();
    if constexpr (PER_SLOT) {
        if (raw.table && rsets) {            // the slots mix raw sets: the set-per-slot forms, `raw` saying which
            with_pattern(layout, [&](auto p) {
                with_stages(raw, [&](auto st) {
                    constexpr int P = decltype(p)::value, ST = decltype(st)::value;
                    auto k_walk = src.tab ? k_rawset_walk_rows<P, SRC_SURFACES, ST> : k_rawset_walk_rows<P, SRC_SLOTS, ST>;
                    if constexpr ((ST & 1) != 0) {
                        if (raw.pack == ma::PACK10) k_walk = src.tab ? k_packset_walk_rows<P, SRC_SURFACES, ST, ma::PACK10> : k_packset_walk_rows<P, SRC_SLOTS, ST, ma::PACK10>;
                        else if (raw.pack == ma::PACK12) k_walk = src.tab ? k_packset_walk_rows<P, SRC_SURFACES, ST, ma::PACK12> : k_packset_walk_rows<P, SRC_SLOTS, ST, ma::PACK12>;
                    }
                    hipLaunchKernelGGL(k_walk, grid, dim3(256), raw_dynamic_lds(raw), s, src.tab, src.frames, src.stride, sets, ids, g, und, und_px,
                                       first_slot, n, remap, rsets, rids, raw.bits);
                });
            });
            return;
        }
    }
    if (raw.table) {
        with_pattern(layout, [&](auto p) {
            with_stages(raw, [&](auto st) {
                constexpr int P = decltype(p)::value, ST = decltype(st)::value;
                auto k_walk = src.tab ? k_raw_walk_rows<P, SRC_SURFACES, PER_SLOT, ST> : k_raw_walk_rows<P, SRC_SLOTS, PER_SLOT, ST>;
                if constexpr ((ST & 1) != 0) {           // MIPI-packed samples: the packed form of the same walk
                    if (raw.pack == ma::PACK10) k_walk = src.tab ? k_mipi_walk_rows<P, SRC_SURFACES, PER_SLOT, ST, ma::PACK10> : k_mipi_walk_rows<P, SRC_SLOTS, PER_SLOT, ST, ma::PACK10>;
                    else if (raw.pack == ma::PACK12) k_walk = src.tab ? k_mipi_walk_rows<P, SRC_SURFACES, PER_SLOT, ST, ma::PACK12> : k_mipi_walk_rows<P, SRC_SLOTS, PER_SLOT, ST, ma::PACK12>;
                }
                hipLaunchKernelGGL(k_walk, grid, dim3(256), raw_dynamic_lds(raw), s, src.tab, src.frames, src.stride, uxy, ufrac, sets, ids, g, und, und_px,
                                   first_slot, n, fpb, remap, raw);
            });
        });
        return;
    }
    with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        auto launch = [&](auto k_walk) {
            hipLaunchKernelGGL(k_walk, grid, dim3(256), 0, s, src.tab, src.frames, src.stride, k, uxy, ufrac, sets, ids, g, und, und_px, first_slot, n, fpb, remap);
        };
        if (src.tab) launch(k_undistort_rows<L, SRC_SURFACES, PER_SLOT>);
        else if (L != 0 || aligned) launch(k_undistort_rows<L, SRC_SLOTS, PER_SLOT>);
        else launch(k_undistort_rows<0, SRC_SLOTS_ANY_BYTE, PER_SLOT>);
    });
}

void launch_undistort_rows(hipStream_t s, FrameSource src, int layout, YuvCoef k, const int16_t* uxy, const uint16_t* ufrac,
                           FrontEndGeom g, uint32_t* und, size_t und_px, int first_slot, int n, const RawStages& raw) {
    if (n <= 0 || g.nrows <= 0) return;
    int fpb = frames_per_thread(n);
    // the slots of a walk are addressed by a 32-bit offset into one buffer resource: a walk stays below 2^30 bytes (one frame
    // per thread where a single frame is larger)
    if (!src.tab) fpb = (int)std::max<size_t>(1, std::min<size_t>((size_t)fpb, (((size_t)1 << 30) - 1) / src.stride));
    const dim3 grid((g.img_w + 255) / 256, g.nrows, (n + fpb - 1) / fpb);
    static const bool unaligned = [] { const char* e = LT_EXP_ENV("LT_UNDISTORT_UNALIGNED"); return e && e[0] == '1'; }();   // A/B
    launch_walk<false>(s, grid, src, layout, k, uxy, ufrac, nullptr, CalIds{}, g, und, und_px, first_slot, n, fpb, unaligned, raw);
}

// The row conversion of n frames in `layout` (not 0), dense or from surfaces: the 16-column kernel where the width and every base and
// pitch of the launch (`bits`: all of them ORed) are multiples of 16, the byte-wise one otherwise; behind a raw table the raw kernel, in the
// same two launch shapes.  MIPI-packed rows (raw.pack) are read in dwords: multiples of 4 there, of 16 on the RGB side.
template <bool SURF, class Src>
static void launch_rows_to_rgb(hipStream_t s, int layout, const Src& src, size_t bits, YuvCoef k, uint8_t* rgb, size_t rgb_stride, int h, int w,
                               int r0, int r1, int n, const RawStages& raw, const RawSetEntry* rsets = nullptr, const uint8_t* rids = nullptr) {
    const bool packed = raw.table && raw.pack >= 0;
    const bool wide = (w & 15) == 0 && (packed ? (bits & 3) == 0 && ((rgb_stride | (size_t)(uintptr_t)rgb) & 15) == 0 : (bits & 15) == 0);
    const dim3 block(wide ? 64 : 256);
    if (raw.table && rids) {                 // the frames mix raw sets (n <= CalIds::N): the set-per-slot forms, `raw` saying which
        const dim3 grid((unsigned)(wide ? (w / 16 + 63) / 64 : (w + 255) / 256), (unsigned)(r1 - r0), (unsigned)n);
        const CalIds ci = pack_ids(rids, n);
        with_pattern(layout, [&](auto p) {
            with_stages(raw, [&](auto st) {
                constexpr int P = decltype(p)::value, ST = decltype(st)::value;
                auto k_rows = wide ? k_rawset_rows_rgb<P, SURF, true, ST> : k_rawset_rows_rgb<P, SURF, false, ST>;
                if constexpr ((ST & 1) != 0) {
                    if (raw.pack == ma::PACK10) k_rows = wide ? k_packset_rows_rgb<P, SURF, true, ST, ma::PACK10> : k_packset_rows_rgb<P, SURF, false, ST, ma::PACK10>;
                    else if (raw.pack == ma::PACK12) k_rows = wide ? k_packset_rows_rgb<P, SURF, true, ST, ma::PACK12> : k_packset_rows_rgb<P, SURF, false, ST, ma::PACK12>;
                }
                hipLaunchKernelGGL(k_rows, grid, block, raw_dynamic_lds(raw), s, src, rgb, rgb_stride, w, r0, h, rsets, ci, raw.bits);
            });
        });
        return;
    }
    if (raw.table) {
        const dim3 grid((unsigned)(wide ? (w / 16 + 63) / 64 : (w + 255) / 256), (unsigned)(r1 - r0), (unsigned)n);
        with_pattern(layout, [&](auto p) {
            with_stages(raw, [&](auto st) {
                constexpr int P = decltype(p)::value, ST = decltype(st)::value;
                auto k_rows = wide ? k_raw_rows_rgb<P, SURF, true, ST> : k_raw_rows_rgb<P, SURF, false, ST>;
                if constexpr ((ST & 1) != 0) {           // MIPI-packed samples: the packed form of the same kernel
                    if (raw.pack == ma::PACK10) k_rows = wide ? k_mipi_rows_rgb<P, SURF, true, ST, ma::PACK10> : k_mipi_rows_rgb<P, SURF, false, ST, ma::PACK10>;
                    else if (raw.pack == ma::PACK12) k_rows = wide ? k_mipi_rows_rgb<P, SURF, true, ST, ma::PACK12> : k_mipi_rows_rgb<P, SURF, false, ST, ma::PACK12>;
                }
                hipLaunchKernelGGL(k_rows, grid, block, raw_dynamic_lds(raw), s, src, rgb, rgb_stride, w, r0, h, raw);
            });
        });
        return;
    }
    with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        if constexpr (L != 0) {
            typedef RowsOf<L> D;
            const unsigned rows = (unsigned)(D::CHROMA_ROWS ? ((r1 + 1) >> 1) - (r0 >> 1) : r1 - r0);
            const dim3 grid((unsigned)(wide ? (w / 16 + 63) / 64 : (w / D::ANY_COLS + 255) / 256), rows, (unsigned)n);
            auto k_rows = wide ? k_rows_to_rgb<L, SURF, true> : k_rows_to_rgb<L, SURF, false>;
            hipLaunchKernelGGL(k_rows, grid, block, 0, s, src, rgb, rgb_stride, w, r0, r1, h, k);
        }
    });
}

void launch_yuv_rows_to_rgb(hipStream_t s, int layout, const uint8_t* yuv, size_t yuv_stride, YuvCoef k, uint8_t* rgb,
                            size_t rgb_stride, int h, int w, int r0, int r1, int n, const RawStages& raw, const RawSetEntry* rsets, const uint8_t* rids) {
    if (n <= 0 || r1 <= r0) return;
    if (raw.table && rids) {                 // the set-per-slot forms: CalIds::N frames per launch
        for (int i = 0; i < n; i += CalIds::N) {
            const int m = std::min(n - i, (int)CalIds::N);
            const uint8_t* src = yuv + (size_t)i * yuv_stride;
            uint8_t* dst = rgb + (size_t)i * rgb_stride;
            launch_rows_to_rgb<false>(s, layout, DenseFrames{src, yuv_stride}, yuv_stride | rgb_stride | (size_t)(uintptr_t)src | (size_t)(uintptr_t)dst, k,
                                      dst, rgb_stride, h, w, r0, r1, m, raw, rsets, rids + i);
        }
        return;
    }
    launch_rows_to_rgb<false>(s, layout, DenseFrames{yuv, yuv_stride}, yuv_stride | rgb_stride | (size_t)(uintptr_t)yuv | (size_t)(uintptr_t)rgb, k,
                              rgb, rgb_stride, h, w, r0, r1, n, raw);
}

void launch_shade_expand(hipStream_t s, const uint16_t* mesh, int mw, int mh, int pattern, uint16_t* plane, int h, int w) {
    hipLaunchKernelGGL(k_shade_expand, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, s, mesh, mw, mh, pattern & 3, plane, h, w);
}

void launch_write_surf_entries(hipStream_t s, SurfEntry* tab, int first, const SurfEntry* entries, int n) {
    for (int i = 0; i < n; i += SurfChunk::N) {
        const int m = std::min(n - i, (int)SurfChunk::N);
        SurfChunk ch{};
        std::copy(entries + i, entries + i + m, ch.e);
        hipLaunchKernelGGL(k_write_surf_entries, dim3(1), dim3(64), 0, s, tab, first + i, m, ch);
    }
}

void launch_surf_rows_to_rgb(hipStream_t s, int layout, const SurfEntry* entries, YuvCoef k, uint8_t* rgb, size_t rgb_stride, int h, int w,
                             int r0, int r1, int n, const RawStages& raw, const RawSetEntry* rsets, const uint8_t* rids) {
    if (n <= 0 || r1 <= r0) return;
    for (int i = 0; i < n; i += SurfChunk::N) {
        const int m = std::min(n - i, (int)SurfChunk::N);
        SurfChunk ch{};
        std::copy(entries + i, entries + i + m, ch.e);
        uint8_t* dst = rgb + (size_t)i * rgb_stride;
        size_t bits = rgb_stride | (size_t)(uintptr_t)dst;   // every base and pitch of the launch a multiple of 16?
        for (int j = 0; j < m; ++j) {
            bits |= (size_t)ch.e[j].plane[0] | (size_t)ch.e[j].pitch;
            if (layout == 1 || layout == 2) bits |= (size_t)ch.e[j].plane[1] | (size_t)ch.e[j].cpitch;
            if (layout == 2) bits |= (size_t)ch.e[j].plane[2];
        }
        if (layout == 0) {
            const int row_bytes = w * 3;
            if ((bits & 15) == 0 && (row_bytes & 15) == 0)
                hipLaunchKernelGGL(k_surf_copy_rows<true>, dim3((unsigned)((row_bytes / 16 + 255) / 256), (unsigned)(r1 - r0), (unsigned)m), dim3(256), 0, s, ch, dst, rgb_stride, row_bytes, r0);
            else
                hipLaunchKernelGGL(k_surf_copy_rows<false>, dim3((unsigned)((row_bytes + 255) / 256), (unsigned)(r1 - r0), (unsigned)m), dim3(256), 0, s, ch, dst, rgb_stride, row_bytes, r0);
        } else {
            launch_rows_to_rgb<true>(s, layout, ch, bits, k, dst, rgb_stride, h, w, r0, r1, m, raw, rsets, rids ? rids + i : nullptr);
        }
    }
}

void launch_warp_split(hipStream_t s, const uint32_t* und, size_t und_px, int first_slot, const int16_t* wxy,
                       const uint16_t* wfrac, FrontEndGeom g, const uint16_t* gamma_tab, const uint16_t* cbrt_tab,
                       const int32_t* coeffs, bool lab_clamp_dead, uint8_t* planeR, uint8_t* planeB, size_t plane_stride, int n) {
    if (n <= 0 || g.nrows <= 0) return;
    const size_t npix = (size_t)g.warp_h * g.warp_w;
    if ((g.warp_w & 3) == 0 && (plane_stride & 3) == 0) {
        const int pairs = ((first_slot + n + 1) >> 1) - (first_slot >> 1);
        const int ppb = std::max(1, frames_per_thread(n) / 2);
        dim3 grid((unsigned)(((npix >> 2) + 255) / 256), 1, (pairs + ppb - 1) / ppb);
        hipLaunchKernelGGL(lab_clamp_dead ? k_warp_split4<false> : k_warp_split4<true>, grid, dim3(256), 0, s, und, und_px, first_slot, wxy,
                           wfrac, g, gamma_tab, cbrt_tab, coeffs, planeR, planeB, plane_stride, n, ppb, xcd_remap());
    } else {
        dim3 grid((unsigned)((npix + 255) / 256), 1, n);
        hipLaunchKernelGGL(k_warp_split1, grid, dim3(256), 0, s, und, und_px, first_slot, wxy, wfrac, g, gamma_tab, cbrt_tab,
                           coeffs, planeR, planeB, plane_stride);
    }
}

void launch_undistort_cal(hipStream_t s, FrameSource src, int layout, YuvCoef k, const CalTables* sets, const uint8_t* ids,
                          FrontEndGeom g, uint32_t* und, size_t und_px, int first_slot, int n, const RawStages& raw, const RawSetEntry* rsets,
                          const uint8_t* rids) {
    if (n <= 0 || g.nrows <= 0) return;
    for (int i = 0; i < n; i += CalIds::N) {
        const int m = std::min(n - i, (int)CalIds::N);
        const dim3 grid((g.img_w + 255) / 256, g.nrows, m);
        const FrameSource part = src.tab ? src : FrameSource::slots(src.frames + (size_t)i * src.stride, src.stride);
        launch_walk<true>(s, grid, part, layout, k, nullptr, nullptr, sets, pack_ids(ids + i, m), g, und, und_px, first_slot + i, m, 1, false, raw,
                          rids ? rsets : nullptr, rids ? pack_ids(rids + i, m) : CalIds{});
    }
}

void launch_warp_cal(hipStream_t s, const uint32_t* und, size_t und_px, int first_slot, const CalTables* sets, const uint8_t* ids,
                     FrontEndGeom g, const uint16_t* gamma_tab, const uint16_t* cbrt_tab, const int32_t* coeffs, uint8_t* planeR,
                     uint8_t* planeB, size_t plane_stride, int n) {
    if (n <= 0 || g.nrows <= 0) return;
    const size_t npix = (size_t)g.warp_h * g.warp_w;
    const bool four = (g.warp_w & 3) == 0 && (plane_stride & 3) == 0;
    for (int i = 0; i < n; i += CalIds::N) {
        const int m = std::min(n - i, (int)CalIds::N);
        const CalIds ci = pack_ids(ids + i, m);
        uint8_t *pr = planeR + (size_t)i * plane_stride, *pb = planeB + (size_t)i * plane_stride;
        if (four)
            hipLaunchKernelGGL(k_warp_cal<4>, dim3((unsigned)(((npix >> 2) + 255) / 256), 1, m), dim3(256), 0, s, und, und_px, first_slot + i,
                               sets, ci, g, gamma_tab, cbrt_tab, coeffs, pr, pb, plane_stride);
        else
            hipLaunchKernelGGL(k_warp_cal<1>, dim3((unsigned)((npix + 255) / 256), 1, m), dim3(256), 0, s, und, und_px, first_slot + i,
                               sets, ci, g, gamma_tab, cbrt_tab, coeffs, pr, pb, plane_stride);
    }
}

void launch_split_bev(hipStream_t s, const uint8_t* bev, size_t bev_stride, int npix, const uint16_t* gamma_tab,
                      const uint16_t* cbrt_tab, const int32_t* coeffs, uint8_t* planeR, uint8_t* planeB,
                      size_t plane_stride, int n) {
    if (n <= 0) return;
    dim3 grid((unsigned)((npix + 255) / 256), 1, n);
    hipLaunchKernelGGL(k_split_bev, grid, dim3(256), 0, s, bev, bev_stride, npix, gamma_tab, cbrt_tab, coeffs, planeR,
                       planeB, plane_stride);
}

void launch_undistorted_to_rgb(hipStream_t s, const uint32_t* und, size_t und_px, int first_slot, int nrows, int w, uint8_t* out,
                               int n) {
    if (n <= 0 || nrows <= 0) return;
    dim3 grid((unsigned)(((size_t)nrows * w + 255) / 256), 1, n);
    hipLaunchKernelGGL(k_undistorted_to_rgb, grid, dim3(256), 0, s, und, und_px, first_slot, nrows, w, out);
}

// Code objects load on the first launch of one of their kernels (a few ms each, once per process and device): lt_create launches
// this no-op so that no stream's first window pays for it (lt_api.cpp: preload_kernels).
namespace { __global__ void k_preload_k_frontend() {} }
void preload_k_frontend(hipStream_t s) { hipLaunchKernelGGL(k_preload_k_frontend, dim3(1), dim3(1), 0, s); }

}  // namespace lt

