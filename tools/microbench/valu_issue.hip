// VALU issue-rate calibration for gfx950: wave-instructions per cycle per SIMD for the integer / packed-16 /
// DPP / permute instructions the mask-stage kernels are made of, and for the fp32 / conversion forms the front end chose its
// blend and Lab tail from (profiles/front_f32_valu_issue.txt), as independent and dependent chains at
// 1..8 waves per SIMD.  Prints one JSON document; tools/microbench/run.sh stores it under profiles/.
//
//   build: hipcc -O2 --offload-arch=gfx950 valu_issue.hip -o valu_issue
//   run:   valu_issue [iters [row,row,...]]      (a list of row names: time these rows only)
//
// Method: a 256-thread workgroup = one wave per SIMD; `W` workgroups per CU are forced by a dynamic-LDS request of
// floor(160 KiB / W) per workgroup, grid = CUs x W (all resident at once).  Each wave executes ITERS x 64 copies of
// one instruction (inline asm, so nothing is folded), bracketed by s_memtime; the slowest wave's cycle count and the
// hipEvent wall time give   rate = W x ITERS x 64 / cycles   [wave-insts / cycle / SIMD].
// A SIMD that needs 4 cycles per wave64 instruction (16 lanes/clk) saturates at 0.25, a 2-cycle SIMD at 0.5.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); std::exit(1); } } while (0)

// eight independent accumulators %0..%7, two read-only operands %8, %9
#define REP8(INS) INS(0) INS(1) INS(2) INS(3) INS(4) INS(5) INS(6) INS(7)
#define DEP8(INS) INS(0) INS(0) INS(0) INS(0) INS(0) INS(0) INS(0) INS(0)
#define X8(B) B B B B B B B B

#define I_PKMIN3(i)  "v_pk_minimum3_f16 %" #i ", %" #i ", %8, %9\n\t"
#define I_PKMAX3(i)  "v_pk_maximum3_f16 %" #i ", %" #i ", %8, %9\n\t"
#define I_PKMAD(i)   "v_pk_mad_u16 %" #i ", %" #i ", %8, %9\n\t"
#define I_PKADD(i)   "v_pk_add_u16 %" #i ", %" #i ", %8\n\t"
#define I_PKSUBI(i)  "v_pk_sub_i16 %" #i ", %" #i ", %8\n\t"
#define I_PKMAXU(i)  "v_pk_max_u16 %" #i ", %" #i ", %8\n\t"
#define I_PKMINU(i)  "v_pk_min_u16 %" #i ", %" #i ", %8\n\t"
#define I_PKLSHR(i)  "v_pk_lshrrev_b16 %" #i ", 1, %" #i "\n\t"
#define I_PERM(i)    "v_perm_b32 %" #i ", %" #i ", %8, %9\n\t"
#define I_DPPROW(i)  "v_mov_b32_dpp %" #i ", %" #i " row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
#define I_DPPWAVE(i) "v_mov_b32_dpp %" #i ", %" #i " wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
#define I_ADDDPP(i)  "v_add_u32_dpp %" #i ", %" #i ", %8 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
#define I_ADD(i)     "v_add_u32 %" #i ", %" #i ", %8\n\t"
#define I_ADD3(i)    "v_add3_u32 %" #i ", %" #i ", %8, %9\n\t"
#define I_ANDOR(i)   "v_and_or_b32 %" #i ", %" #i ", %8, %9\n\t"
#define I_LSHLOR(i)  "v_lshl_or_b32 %" #i ", %" #i ", 1, %9\n\t"
#define I_SAD(i)     "v_sad_u8 %" #i ", %" #i ", %8, %9\n\t"
#define I_MAD24(i)   "v_mad_u32_u24 %" #i ", %" #i ", %8, %9\n\t"
#define I_MULLO(i)   "v_mul_lo_u32 %" #i ", %" #i ", %8\n\t"
#define I_ALIGN(i)   "v_alignbit_b32 %" #i ", %" #i ", %8, 8\n\t"
#define I_BFE(i)     "v_bfe_u32 %" #i ", %" #i ", 1, 30\n\t"
#define I_MIN3U(i)   "v_min3_u32 %" #i ", %" #i ", %8, %9\n\t"
#define I_FMA(i)     "v_fma_f32 %" #i ", %" #i ", %8, %9\n\t"
#define I_PKFMA(i)   "v_pk_fma_f16 %" #i ", %" #i ", %8, %9\n\t"
#define I_CNDMASK(i) "v_cndmask_b32 %" #i ", %" #i ", %8, vcc\n\t"
#define I_CMP16(i)   "v_cmp_gt_i16 vcc, %" #i ", %8\n\t"
#define I_CMP32S(i)  "v_cmp_lt_i32_e64 s[20:21], %" #i ", %8\n\t"
#define I_WRLANE(i)  "v_writelane_b32 %" #i ", s20, 5\n\t"
#define I_LSHL64(i)  "v_lshlrev_b32 %" #i ", 1, %" #i "\n\t"
#define I_XOR(i)     "v_xor_b32 %" #i ", %" #i ", %8\n\t"
#define I_BFI(i)     "v_bfi_b32 %" #i ", %" #i ", %8, %9\n\t"
#define I_MOV(i)     "v_mov_b32 %" #i ", %8\n\t"
#define I_MBCNT(i)   "v_mbcnt_lo_u32_b32 %" #i ", %8, %" #i "\n\t"
#define I_AND(i)     "v_and_b32 %" #i ", %" #i ", %8\n\t"
#define I_OR(i)      "v_or_b32 %" #i ", %" #i ", %8\n\t"
#define I_SUB(i)     "v_sub_u32 %" #i ", %" #i ", %8\n\t"
#define I_MINU(i)    "v_min_u32 %" #i ", %" #i ", %8\n\t"
#define I_MAXU(i)    "v_max_u32 %" #i ", %" #i ", %8\n\t"
#define I_MAXI16(i)  "v_max_i16 %" #i ", %" #i ", %8\n\t"
#define I_ADD16(i)   "v_add_u16 %" #i ", %" #i ", %8\n\t"
#define I_MUL24(i)   "v_mul_u32_u24 %" #i ", %" #i ", %8\n\t"
#define I_LSHR(i)    "v_lshrrev_b32 %" #i ", 1, %" #i "\n\t"
#define I_ASHR(i)    "v_ashrrev_i32 %" #i ", 1, %" #i "\n\t"
#define I_ADDSDWA(i) "v_add_u32_sdwa %" #i ", %" #i ", %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\t"
#define I_ADDCO(i)   "v_add_co_u32 %" #i ", vcc, %" #i ", %8\n\t"
#define I_ADDF(i)    "v_add_f32 %" #i ", %" #i ", %8\n\t"
#define I_PKADDF16(i) "v_pk_add_f16 %" #i ", %" #i ", %8\n\t"
#define I_PKMULLO(i) "v_pk_mul_lo_u16 %" #i ", %" #i ", %8\n\t"
#define I_MADU16(i)  "v_mad_u16 %" #i ", %" #i ", %8, %9\n\t"
#define I_BFREV(i)   "v_bfrev_b32 %" #i ", %" #i "\n\t"
#define I_CNDADD(i)  "v_cndmask_b32 %" #i ", %" #i ", %8, vcc\n\tv_add_u32 %" #i ", %" #i ", %8\n\tv_add_u32 %" #i ", %" #i ", %9\n\tv_add_u32 %" #i ", %" #i ", %8\n\t"
#define I_CNDS(i)    "v_cndmask_b32 %" #i ", %" #i ", %8, s[20:21]\n\t"
#define I_PERMADD(i) "v_perm_b32 %" #i ", %" #i ", %8, %9\n\tv_add_u32 %" #i ", %" #i ", %8\n\t"
#define I_READLANE(i) "v_readlane_b32 s20, %" #i ", 3\n\t"
// the fp32 / conversion forms the front end's blend and Lab tail choose from (profiles/front_f32_valu_issue.txt)
#define I_CVTUB0(i)  "v_cvt_f32_ubyte0_e32 %" #i ", %" #i "\n\t"
#define I_CVTUB1(i)  "v_cvt_f32_ubyte1_e32 %" #i ", %" #i "\n\t"
#define I_CVTUB2(i)  "v_cvt_f32_ubyte2_e32 %" #i ", %" #i "\n\t"
#define I_CVTUB3(i)  "v_cvt_f32_ubyte3_e32 %" #i ", %" #i "\n\t"
#define I_CVTFU(i)   "v_cvt_f32_u32_e32 %" #i ", %" #i "\n\t"
#define I_CVTUF(i)   "v_cvt_u32_f32_e32 %" #i ", %" #i "\n\t"
#define I_FLOOR(i)   "v_floor_f32_e32 %" #i ", %" #i "\n\t"
#define I_FMAC(i)    "v_fmac_f32_e32 %" #i ", %8, %9\n\t"
#define I_MULF(i)    "v_mul_f32_e32 %" #i ", %" #i ", %8\n\t"
#define I_MINF(i)    "v_min_f32_e32 %" #i ", %" #i ", %8\n\t"
#define I_MAXF(i)    "v_max_f32_e32 %" #i ", %" #i ", %8\n\t"
#define I_MED3F(i)   "v_med3_f32 %" #i ", %" #i ", %8, %9\n\t"
#define I_MINU16(i)  "v_min_u16_e32 %" #i ", %" #i ", %8\n\t"
#define I_MINI16(i)  "v_min_i16_e32 %" #i ", %" #i ", %8\n\t"
#define I_MAXU16(i)  "v_max_u16_e32 %" #i ", %" #i ", %8\n\t"
#define I_CVTPKU8(i) "v_cvt_pk_u8_f32 %" #i ", %" #i ", %8, %9\n\t"
#define I_DOT2U16(i) "v_dot2_u32_u16 %" #i ", %" #i ", %8, %9\n\t"
#define I_LSHL_E32(i) "v_lshlrev_b32_e32 %" #i ", 1, %" #i "\n\t"
#define I_LSHL_E64(i) "v_lshlrev_b32_e64 %" #i ", 1, %" #i "\n\t"
#define I_LSHR_E64(i) "v_lshrrev_b32_e64 %" #i ", 1, %" #i "\n\t"
// packed fp32: every operand is a 64-bit register pair (OPS64)
#define I_PKFMAF32(i) "v_pk_fma_f32 %" #i ", %" #i ", %8, %9\n\t"
#define I_PKMULF32(i) "v_pk_mul_f32 %" #i ", %" #i ", %8\n\t"
#define I_PKADDF32(i) "v_pk_add_f32 %" #i ", %" #i ", %8\n\t"

#define OPS(F) \
    F(pk_minimum3_f16, I_PKMIN3) F(pk_maximum3_f16, I_PKMAX3) F(pk_mad_u16, I_PKMAD) F(pk_add_u16, I_PKADD) \
    F(pk_sub_i16, I_PKSUBI) F(pk_max_u16, I_PKMAXU) F(pk_min_u16, I_PKMINU) F(pk_lshrrev_b16, I_PKLSHR) F(perm_b32, I_PERM) \
    F(mov_dpp_row_shr1, I_DPPROW) F(mov_dpp_wave_shr1, I_DPPWAVE) F(add_u32_dpp_row_shr1, I_ADDDPP) F(add_u32, I_ADD) \
    F(add3_u32, I_ADD3) F(and_or_b32, I_ANDOR) F(lshl_or_b32, I_LSHLOR) F(sad_u8, I_SAD) F(mad_u32_u24, I_MAD24) \
    F(mul_lo_u32, I_MULLO) F(alignbit_b32, I_ALIGN) F(bfe_u32, I_BFE) F(min3_u32, I_MIN3U) F(fma_f32, I_FMA) \
    F(pk_fma_f16, I_PKFMA) F(cndmask_b32, I_CNDMASK) F(cmp_gt_i16_vcc, I_CMP16) F(cmp_lt_i32_sgpr, I_CMP32S) \
    F(writelane_b32, I_WRLANE) F(lshlrev_b32, I_LSHL64) F(xor_b32, I_XOR) F(bfi_b32, I_BFI) F(mov_b32, I_MOV) \
    F(mbcnt_lo, I_MBCNT) F(and_b32, I_AND) F(or_b32, I_OR) F(sub_u32, I_SUB) F(min_u32, I_MINU) F(max_u32, I_MAXU) \
    F(max_i16, I_MAXI16) F(add_u16, I_ADD16) F(mul_u32_u24, I_MUL24) F(lshrrev_b32, I_LSHR) F(ashrrev_i32, I_ASHR) \
    F(add_u32_sdwa_byte, I_ADDSDWA) F(add_co_u32, I_ADDCO) F(add_f32, I_ADDF) F(pk_add_f16, I_PKADDF16) \
    F(pk_mul_lo_u16, I_PKMULLO) F(mad_u16, I_MADU16) F(bfrev_b32, I_BFREV) F(cndmask_then_3_adds_x4insts, I_CNDADD) \
    F(cndmask_sgpr_mask, I_CNDS) F(perm_then_add_x2insts, I_PERMADD) F(readlane_b32, I_READLANE) \
    F(cvt_f32_ubyte0, I_CVTUB0) F(cvt_f32_ubyte1, I_CVTUB1) F(cvt_f32_ubyte2, I_CVTUB2) F(cvt_f32_ubyte3, I_CVTUB3) \
    F(cvt_f32_u32, I_CVTFU) F(cvt_u32_f32, I_CVTUF) F(floor_f32, I_FLOOR) F(fmac_f32_e32, I_FMAC) F(mul_f32, I_MULF) \
    F(min_f32, I_MINF) F(max_f32, I_MAXF) F(med3_f32, I_MED3F) F(min_u16_e32, I_MINU16) F(min_i16_e32, I_MINI16) \
    F(max_u16_e32, I_MAXU16) F(cvt_pk_u8_f32, I_CVTPKU8) F(dot2_u32_u16, I_DOT2U16) F(lshlrev_b32_e32, I_LSHL_E32) \
    F(lshlrev_b32_e64, I_LSHL_E64) F(lshrrev_b32_e64, I_LSHR_E64)
#define OPS64(F) F(pk_fma_f32, I_PKFMAF32) F(pk_mul_f32, I_PKMULF32) F(pk_add_f32, I_PKADDF32)

extern "C" __global__ void k_dummy() {}

#define DEFINE_KERNEL(NAME, INS) DEFINE_KERNEL_T(NAME, INS, unsigned)
#define DEFINE_KERNEL64(NAME, INS) DEFINE_KERNEL_T(NAME, INS, unsigned long long)
#define DEFINE_KERNEL_T(NAME, INS, T)                                                                                   \
    template <bool DEP>                                                                                              \
    __global__ __launch_bounds__(256) void k_##NAME(int iters, unsigned long long* cycles, unsigned* sink) {         \
        extern __shared__ unsigned char smem_[];                                                                     \
        T a0 = threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6,           \
          a7 = a0 + 7;                                                                                               \
        const T b = 0x00030005u + (threadIdx.x & 1), c = 0x04020400u;                                                \
        __syncthreads();                                                                                             \
        const unsigned long long t0 = __builtin_readcyclecounter();                                                  \
        for (int it = 0; it < iters; ++it) {                                                                         \
            if (DEP)                                                                                                 \
                asm volatile(X8(DEP8(INS))                                                                           \
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)        \
                             : "v"(b), "v"(c)                                                                        \
                             : "vcc", "s20", "s21");                                                                 \
            else                                                                                                     \
                asm volatile(X8(REP8(INS))                                                                           \
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)        \
                             : "v"(b), "v"(c)                                                                        \
                             : "vcc", "s20", "s21");                                                                 \
        }                                                                                                            \
        const unsigned long long t1 = __builtin_readcyclecounter();                                                  \
        if ((threadIdx.x & 63) == 0) cycles[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;                          \
        if ((a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7) == 0x12345u) sink[0] = smem_[0];                                 \
    }
OPS(DEFINE_KERNEL)
OPS64(DEFINE_KERNEL64)

struct Op {
    const char* name;
    void (*indep)(int, unsigned long long*, unsigned*);
    void (*dep)(int, unsigned long long*, unsigned*);
};
#define OP_ENTRY(NAME, INS) {#NAME, k_##NAME<false>, k_##NAME<true>},
static const Op g_ops[] = {OPS(OP_ENTRY) OPS64(OP_ENTRY)};

int main(int argc, char** argv) {
    int dev = 0;
    CHECK(hipSetDevice(dev));
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, dev));
    const int cus = prop.multiProcessorCount;
    int clock_khz = 0;
    CHECK(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeClockRate, dev));
    const int iters = argc > 1 ? std::atoi(argv[1]) : 2000;
    const char* only = argc > 2 ? argv[2] : nullptr;   // a comma-separated list of row names: time these rows only
    unsigned long long* d_cycles;
    unsigned* d_sink;
    CHECK(hipMalloc(&d_cycles, sizeof(unsigned long long) * cus * 8 * 4));
    CHECK(hipMalloc(&d_sink, 64));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<unsigned long long> h(cus * 8 * 4);
    const int Ws[] = {1, 2, 3, 4, 5, 6, 8};
    std::printf("{\"device\": \"%s\", \"cus\": %d, \"clock_rate_khz\": %d, \"iters\": %d, \"insts_per_wave\": %d,\n",
                prop.name[0] ? prop.name : prop.gcnArchName, cus, clock_khz, iters, iters * 64);
    std::printf(" \"method\": \"W workgroups of 4 waves per CU (one wave per SIMD each), every wave issues iters*64 copies of one "
                "instruction; rate = W*insts / cycles of the slowest wave (s_memtime), wave-instructions per cycle per SIMD; "
                "ghz = insts*W*4*cus/(rate*... ) see wall_ms\",\n \"ops\": {\n");
    bool first = true;
    for (const Op& op : g_ops) {
        if (only) {
            const std::string list = std::string(",") + only + ",", key = std::string(",") + op.name + ",";
            if (list.find(key) == std::string::npos) continue;
        }
        for (int dep = 0; dep < 2; ++dep) {
            auto fn = dep ? op.dep : op.indep;
            std::printf("%s  \"%s/%s\": {", first ? "" : ",\n", op.name, dep ? "dep" : "indep");
            first = false;
            bool f2 = true;
            for (int W : Ws) {
                const size_t lds = (160 * 1024) / W - 64;
                CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                const int grid = cus * W;
                hipLaunchKernelGGL(fn, dim3(grid), dim3(256), lds, 0, 10, d_cycles, d_sink);   // warm-up
                CHECK(hipDeviceSynchronize());
                CHECK(hipEventRecord(e0));
                hipLaunchKernelGGL(fn, dim3(grid), dim3(256), lds, 0, iters, d_cycles, d_sink);
                CHECK(hipEventRecord(e1));
                CHECK(hipDeviceSynchronize());
                float ms = 0;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                CHECK(hipMemcpy(h.data(), d_cycles, sizeof(unsigned long long) * grid * 4, hipMemcpyDeviceToHost));
                unsigned long long mx = 0, sum = 0;
                for (int i = 0; i < grid * 4; ++i) { mx = std::max(mx, h[i]); sum += h[i]; }
                const double insts = (double)iters * 64.0;
                const double rate_max = W * insts / (double)mx, rate_avg = W * insts / ((double)sum / (grid * 4));
                // wall-clock rate: wave-insts per ns per SIMD -> divide by GHz to compare; report raw
                const double per_ns = W * insts / (ms * 1e6);
                std::printf("%s\"%d\": {\"rate\": %.4f, \"rate_avg_wave\": %.4f, \"wave_insts_per_ns_per_simd\": %.4f, \"wall_ms\": %.4f}",
                            f2 ? "" : ", ", W, rate_max, rate_avg, per_ns, ms);
                f2 = false;
            }
            std::printf("}");
            std::fflush(stdout);
        }
    }
    std::printf("\n }\n}\n");
    return 0;
}
