// Shot noise: a Poisson draw per element from the counter-based generator of common.h.  Every decision of a
// draw is evaluated in float64 and depends on (seed, stream, sample, element) alone, so chunked, repeated and in-place calls give the
// same bits and tests/poisson_ref.py can restate it element by element.  Built with -ffp-contract=off: every operation is rounded
// separately, as numpy rounds it.
#include <math.h>
#include "common.h"

#define POISSON_SMALL 10.0             // below: inversion, from here on: PTRS
#define POISSON_RATE_MAX 1073741824.0  // 2^30; above (and for a negative or NaN rate): NaN
#define POISSON_MAX_STEPS 80           // inversion: P(k > 80 | rate < 10) is far below the 2^-33 resolution of u
#define POISSON_MAX_ROUNDS 32          // PTRS: 64 attempts, then rint(rate)

// u = (r + 0.5) * 2^-32: exact in float64, strictly inside (0, 1)
__device__ __forceinline__ double poisson_u01(uint32_t r) { return ((double)r + 0.5) * 2.3283064365386963e-10; }

// the block of round t: counter (e & 0xffffffff, (e >> 32) | (t << 20), sample, stream_id); e < 2^52 keeps the two fields apart
__device__ __forceinline__ u32x4 poisson_block(uint64_t e, uint32_t t, uint32_t sample, uint32_t stream_id, uint32_t k0, uint32_t k1) {
    return cwfa_philox4x32_10((uint32_t)e, (uint32_t)(e >> 32) | (t << 20), sample, stream_id, k0, k1);
}

// k ~ Poisson(rate) as a double (an integer <= about 2^30 + 2^18), NaN for a refused rate
__device__ __forceinline__ double poisson_draw(float rate_f, uint64_t e, uint32_t sample, uint32_t stream_id, uint32_t k0, uint32_t k1) {
    const double rate = (double)rate_f;
    if (!(rate >= 0.0) || rate > POISSON_RATE_MAX) return __builtin_nan("");
    if (rate < POISSON_SMALL) {
        // inversion by sequential search: rate = 0 gives p = F = 1 >= u, k = 0
        const double u = poisson_u01(poisson_block(e, 0, sample, stream_id, k0, k1)[0]);
        int k = 0;
        double p = exp(-rate), F = p;
        while (u > F && k < POISSON_MAX_STEPS) {
            k += 1;
            p *= rate / (double)k;
            F += p;
        }
        return (double)k;
    }
    // Hoermann's PTRS (transformed rejection with squeeze), the constants of numpy / torch
    const double slam = sqrt(rate), loglam = log(rate);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double inv_alpha = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    for (uint32_t t = 0; t < POISSON_MAX_ROUNDS; ++t) {
        const u32x4 w = poisson_block(e, t, sample, stream_id, k0, k1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double U = poisson_u01(w[2 * h]) - 0.5, V = poisson_u01(w[2 * h + 1]);
            const double us = 0.5 - fabs(U);
            const double k = floor((2.0 * a / us + b) * U + rate + 0.43);
            if (us >= 0.07 && V <= vr) return k;
            if (k < 0.0 || (us < 0.013 && V > us)) continue;
            if (log(V) + log(inv_alpha) - log(a / (us * us) + b) <= -rate + k * loglam - lgamma(k + 1.0)) return k;
        }
    }
    return rint(rate);
}

// out[s][e] = fl32(fl32(k) * post[s]), k ~ Poisson(fl32(lam[s * lam_ss + e] * pre[s])).  blockIdx.y walks the samples, blockIdx.x the
// elements of one; an element reads its own rate only, before its store (in place is safe), and every lane reaches the store.
__global__ __launch_bounds__(256) void rand_poisson_kernel(float* out, const float* lam, int N, int64_t n, int64_t lam_ss, int64_t out_ss,
                                                           const float* __restrict__ pre, const float* __restrict__ post, uint32_t k0,
                                                           uint32_t k1, uint32_t stream_id, uint32_t sample_offset) {
    for (int s = blockIdx.y; s < N; s += gridDim.y) {
        const float* lp = lam + s * lam_ss;
        float* op = out + s * out_ss;
        const float pre_s = pre ? pre[s] : 1.0f, post_s = post ? post[s] : 1.0f;
        const uint32_t sample = sample_offset + (uint32_t)s;
        for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
            const float k = (float)poisson_draw(lp[e] * pre_s, (uint64_t)e, sample, stream_id, k0, k1);      // x * 1 is x
            op[e] = k * post_s;
        }
    }
}

extern "C" int cwfa_rand_poisson_f32(float* out, const float* lam, int N, int64_t n, int64_t lam_ss, int64_t out_ss, const float* pre,
                                     const float* post, uint64_t seed, uint32_t stream_id, uint32_t sample_offset, void* stream) {
    const char* name = "cwfa_rand_poisson_f32";
    CWFA_REQUIRE(out && lam, CWFA_E_INVAL, "%s: null pointer", name);
    CWFA_REQUIRE(N >= 0 && n >= 0, CWFA_E_SHAPE, "%s: bad shape", name);
    CWFA_REQUIRE(n <= ((int64_t)1 << 52), CWFA_E_SHAPE, "%s: %lld elements per sample exceed the 2^52 the counter holds", name, (long long)n);
    CWFA_REQUIRE(N <= 1 || (out_ss >= n && (lam_ss == 0 || lam_ss >= n)), CWFA_E_INVAL,
                 "%s: a sample stride (lam %lld, out %lld) is below the %lld elements of a sample (lam_ss = 0 shares one plane)", name,
                 (long long)lam_ss, (long long)out_ss, (long long)n);
    CWFA_REQUIRE(out != lam || N <= 1 || lam_ss == out_ss, CWFA_E_INVAL, "%s: in place needs lam_ss == out_ss", name);
    if (N == 0 || n == 0) return CWFA_OK;
    // a grid-stride walk: at most 2048 blocks per sample row and 64 rows, enough to fill the chip several times over
    const int64_t want = (n + 255) / 256;
    const unsigned bx = (unsigned)(want < 2048 ? want : 2048), by = (unsigned)(N < 64 ? N : 64);
    hipLaunchKernelGGL(rand_poisson_kernel, dim3(bx, by), dim3(256), 0, (hipStream_t)stream, out, lam, N, n, lam_ss, out_ss, pre, post,
                       (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), stream_id, sample_offset);
    CWFA_LAUNCH_CHECK(name);
    return CWFA_OK;
}
