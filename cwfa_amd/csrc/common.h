// Shared helpers for the libcwfa_hip.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "cwfa_hip.h"

void cwfa_set_error(const char* fmt, ...);

#define CWFA_REQUIRE(cond, code, ...)        \
    do {                                     \
        if (!(cond)) {                       \
            cwfa_set_error(__VA_ARGS__);     \
            return (code);                   \
        }                                    \
    } while (0)

#define CWFA_LAUNCH_CHECK(name)                                              \
    do {                                                                     \
        hipError_t e_ = hipGetLastError();                                   \
        if (e_ != hipSuccess) {                                              \
            cwfa_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
            return CWFA_E_HIP;                                               \
        }                                                                    \
    } while (0)

// vector types of the kernels; lds_ptr: an LDS address (the LDS-DMA destination of __builtin_amdgcn_raw_ptr_buffer_load_lds)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr;

static inline bool cwfa_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// fp32 constant the reference multiplies with: python float 1/math.sqrt(2) rounded to fp32 (INN_utils.py:150,161)
#define CWFA_INV_SQRT2_F 0.70710678118654752440f
// fp32(math.sqrt(2)) used as a divisor in networks.py:671
#define CWFA_SQRT2_F 1.41421356237309504880f

// wave64 sum, result valid in every lane
__device__ __forceinline__ double cwfa_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float cwfa_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the 16 lanes of a DPP row (lanes with equal lane >> 4), result valid in all 16: quad xor 1, quad xor 2, mirror of the
// half row, mirror of the row -- four VALU instructions, no LDS
__device__ __forceinline__ float cwfa_row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}

// Buffer descriptor of `bytes` bytes from `base` (stride 0: raw byte offsets, range-checked against `bytes`; out-of-range
// loads return 0).  Word 3 = 0x00020000: DATA_FORMAT (bits 18:15) = 4, 32-bit, no swizzle, no index stride -- the
// buffer-descriptor recipe of the CDNA HIP programming guide (T8, T20).  Build it from wave-uniform values only.  (A macro:
// behind an inline function the compiler orders the scalar setup of some descriptors differently.)
#define CWFA_RSRC(base, bytes) \
    __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(static_cast<const void*>(base)), 0, (bytes), 0x00020000)

// 16-byte buffer store with an SGPR offset.  gfx950: the store keeps reading its data registers after issue, also in this
// addressing form, which LLVM's hazard rule exempts ("only if soffset is not a register"): a VALU write into the tuple right
// behind it corrupted the stored data.  EVERY 16-byte buffer store of the library goes through
// this helper, which carries the wait states and keeps the scheduler from moving anything across.
__device__ __forceinline__ void cwfa_buffer_store_b128(u32x4 data, __amdgpu_buffer_rsrc_t rsrc, unsigned voffset, int soffset) {
    __builtin_amdgcn_raw_buffer_store_b128(data, rsrc, voffset, soffset, 0);
    asm volatile("s_nop 1");
    __builtin_amdgcn_sched_barrier(0);
}

// block-wide sum of doubles (blockDim.x multiple of 64, <= 1024); result valid in thread 0.
__device__ __forceinline__ double cwfa_block_sum(double v, double* lds /* >= 16 doubles */) {
    v = cwfa_wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < nw; ++i) r += lds[i];
    __syncthreads();
    return r;
}

// ELU(v) = v > 0 ? v : expm1(v).  ocml's expm1f is ~30 VALU instructions, and on gfx950 every vector instruction of an
// fp32-MFMA kernel is time taken from the matrix pipe (they do not co-execute), so: hardware exp (v_exp_f32) minus one,
// 5 instructions.  Absolute error <= 1.2e-7 (one ulp of exp(v) ~ 1); the relative error of tiny negative results is
// not bounded, which the 1e-4 parity bound (relative to the tensor's max) does not need.
__device__ __forceinline__ float cwfa_elu(float v) {
    const float e = __expf(v) - 1.0f;
    return v > 0.f ? v : e;
}
// atan for the soft clamp of the couplings (coupling_layers.py:52: 0.636 * atan(s / clamp) ...).  ocml's atanf is ~30 vector
// instructions (an IEEE division in its range reduction); the fused chain kernels evaluate it five times per element and
// were VALU-bound on it.  Here: r = |x| or 1/|x| (v_rcp_f32), atan(r) = r * P(r^2) with a degree-7 Chebyshev-interpolated
// P on [0, 1], pi/2 - . for |x| > 1, sign restored: 15 instructions, absolute error <= 1.9e-7 (3 ulp at pi/2) over all x.
__device__ __forceinline__ float cwfa_atan(float x) {
    const float ax = fabsf(x);
    const bool inv = ax > 1.0f;
    const float r = inv ? __builtin_amdgcn_rcpf(ax) : ax;
    const float t = r * r;
    float p = -0.00455979211255908f;
    p = fmaf(p, t, 0.023780519142746925f);
    p = fmaf(p, t, -0.05882975459098816f);
    p = fmaf(p, t, 0.09868865460157394f);
    p = fmaf(p, t, -0.14003290235996246f);
    p = fmaf(p, t, 0.19966961443424225f);
    p = fmaf(p, t, -0.3333181142807007f);
    p = fmaf(p, t, 0.9999998807907104f);
    float a = p * r;
    a = inv ? 1.57079632679489661923f - a : a;
    return copysignf(a, x);
}

// tanh for the TANH soft clamp (AllInOneBlock, all_in_one_block.py:216): 1 - 2 / (exp(2x) + 1) on the hardware exp and reciprocal
// for |x| >= 0.35 (absolute error <= 2.5e-7; exp saturates cleanly: +-1 for |x| > 44), and the odd series x P(x^2) below that:
// the first form cancels for small |x| (relative error ~1e-3 at |x| = 1e-4, where freshly initialised AllInOne blocks sit: their
// summed log-det would carry that floor).  Series truncated after x^9: next term 1382/155925 x^11 < 9e-8 x at 0.35.
__device__ __forceinline__ float cwfa_tanh(float x) {
    const float e = __expf(2.0f * x);
    const float big = 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
    const float t = x * x;
    float p = 62.0f / 2835.0f;
    p = fmaf(p, t, -17.0f / 315.0f);
    p = fmaf(p, t, 2.0f / 15.0f);
    p = fmaf(p, t, -1.0f / 3.0f);
    p = fmaf(p, t, 1.0f);
    return fabsf(x) < 0.35f ? x * p : big;
}

__device__ __forceinline__ float cwfa_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

__device__ __forceinline__ float cwfa_act(float v, int act, float alpha) {
    switch (act) {
        case CWFA_ACT_ELU: return cwfa_elu(v);
        case CWFA_ACT_PRELU: return v > 0.f ? v : alpha * v;
        case CWFA_ACT_GELU: return cwfa_gelu(v);
        case CWFA_ACT_RELU: return v > 0.f ? v : 0.f;
        default: return v;
    }
}

// compile-time activation (the epilogues specialised per activation); same cases as cwfa_act
template <int ACT>
__device__ __forceinline__ float cwfa_act_ct(float v, float alpha) {
    if constexpr (ACT == CWFA_ACT_ELU) return cwfa_elu(v);
    if constexpr (ACT == CWFA_ACT_PRELU) return v > 0.f ? v : alpha * v;
    if constexpr (ACT == CWFA_ACT_GELU) return cwfa_gelu(v);
    if constexpr (ACT == CWFA_ACT_RELU) return v > 0.f ? v : 0.f;
    return v;
}

// the soft clamp of the coupling blocks (coupling_layers.py:50-60): the affine apply / chain kernels (elementwise.hip) and the
// coupling epilogue of the split 3x3 (conv_split3x3.hip) both go through this one definition -- their parity rests on it
__device__ __forceinline__ float cwfa_soft_clamp(float a, int kind, float clamp) {
    switch (kind) {
        case CWFA_CLAMP_ATAN: return clamp * (0.636f * cwfa_atan(a));
        case CWFA_CLAMP_TANH: return clamp * cwfa_tanh(a);
        case CWFA_CLAMP_SIGMOID: return clamp * (2.f * (1.f / (1.f + expf(-a)) - 0.5f));
        default: return clamp * a;
    }
}

// ---- the device generator of the samplers (cwfa_rand_*_f32, cwfa_chain_inv_samples_f32).
// Philox4x32-10 (Salmon et al., SC'11; the Random123 known answers are in tests/test_sampler_cpu.py): ten rounds of
//   (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),   key += (0x9E3779B9, 0xBB67AE85)
// The counter convention is part of the interface: element e (the contiguous linear index within one sample) of sample n takes
// word e & 3 of the block with counter (g & 0xffffffff, g >> 32, sample_offset + n, stream_id), g = e >> 2, under the key
// (seed & 0xffffffff, seed >> 32) -- so chunked, repeated and differently dispatched calls draw the same values.
__device__ __forceinline__ u32x4 cwfa_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}
// the Philox block of group g of sample counter `sample` (= sample_offset + n, modulo 2^32)
__device__ __forceinline__ u32x4 cwfa_rand_block(uint64_t g, uint32_t sample, uint32_t stream_id, uint32_t k0, uint32_t k1) {
    return cwfa_philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), sample, stream_id, k0, k1);
}
// u = ((r >> 9) + 0.5) * 2^-23: an odd multiple of 2^-24 below 1, exact in fp32 and strictly inside (0, 1)
__device__ __forceinline__ float cwfa_rand_u01(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 1.1920928955078125e-07f; }
// the map of _no_grad_trunc_normal_ (mean 0, std 1, bounds +-T): E = (float)erf(T / sqrt 2) from the host; 2u - 1 is exact
__device__ __forceinline__ float cwfa_rand_trunc_normal(uint32_t r, float E, float T) {
    const float a = E * (2.0f * cwfa_rand_u01(r) - 1.0f);
    return fminf(fmaxf(CWFA_SQRT2_F * erfinvf(a), -T), T);
}

// a compile-time int argument (read as decltype(k)::value), and f(cwfa_ic<i>{}) for i = 0 .. N-1 unrolled at compile time
template <int K>
using cwfa_ic = std::integral_constant<int, K>;
template <class F, int... I>
__device__ __forceinline__ void cwfa_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(cwfa_ic<I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void cwfa_static_for(F&& f) {
    cwfa_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// channel held by accumulator register r of a 32x32 fp32 MFMA tile in lane half kh (C/D layout of v_mfma_f32_32x32x2_f32)
__device__ __forceinline__ int cwfa_acc_row(int r, int kh) { return (r & 3) + 8 * (r >> 2) + 4 * kh; }

// The three-way bf16 split of the fp32-equivalent kernels: v = a1 + a2 + a3 EXACTLY (24 significand bits; each difference is
// exact: the subtrahend is the minuend rounded to 8 significant bits).  SIX = false: the leading piece only (plain bf16
// operands, `split_products` = 1); a2 and a3 are then not written.
// F16 (`split_operand` = 1, single product only): the one piece is the fp16 value instead, round to nearest even like torch's
// .half() (v_cvt_f16_f32, not the round-toward-zero packed form); beyond +-65504 it is +-inf.  Its bits ride in the __bf16:
// the LDS images and fragments are 16-bit lanes either way, and the F16 MFMA reads them as fp16 (CWFA_MFMA_OP).
template <bool SIX, bool F16 = false>
__device__ __forceinline__ void cwfa_split3(float v, __bf16& a1, __bf16& a2, __bf16& a3) {
    static_assert(!(SIX && F16), "fp16 operands: single product only");
    if constexpr (F16) {
        a1 = __builtin_bit_cast(__bf16, (_Float16)v);
        return;
    }
    a1 = (__bf16)v;
    if constexpr (SIX) {
        const float r1 = v - (float)a1;
        a2 = (__bf16)r1;
        const float r2 = r1 - (float)a2;
        a3 = (__bf16)r2;
    }
}

// c += a . b on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16), and a scheduling barrier no instruction is moved across
#define CWFA_MFMA(a, b, c) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
// the same product with fp16 operands (v_mfma_f32_16x16x32_f16: the A / B fragment layouts of the two forms are the same)
#define CWFA_MFMA_F16(a, b, c) \
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0)
// CWFA_MFMA or CWFA_MFMA_F16 by the kernel's operand format
#define CWFA_MFMA_OP(F16, a, b, c) \
    do {                           \
        if constexpr (F16)         \
            CWFA_MFMA_F16(a, b, c); \
        else                       \
            CWFA_MFMA(a, b, c);    \
    } while (0)
#define CWFA_FENCE() __builtin_amdgcn_sched_barrier(0)
