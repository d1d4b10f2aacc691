// The weighted-MSE training loss (`wL2`: reference losses.py:477-500, chosen by --loss_func_first_step / --loss_func_reg, CWFA.py:936-959):
// an MSE over the voxels brighter than ths_perc of the range in BOTH volumes.  One HBM-bound streaming pass behind
// cwfa_volume_extrema_f32: both tensors read once, the gradient map written once, the sum and the in-mask count reduced in two stages
// (per-block float64 partials in a slab, added in a fixed order: bitwise reproducible).  Built with -ffp-contract=off: the masks are
// the reference's fp32 arithmetic bit for bit.
#include "common.h"

#define WMSE_THREADS 256
#define WMSE_MAX_BLOCKS 2048    // the chip eight times over; a block streams >= 4096 elements
#define WMSE_UNROLL 4           // 16-byte groups per tensor in flight per thread

// the gates as the reference forms them: (v - min) > (max - min) * ths_perc, every operation rounded to fp32
struct wmse_gate {
    float omin, otho, tmin, ttho;
};

static inline int wmse_blocks(int64_t n) {
    int64_t s = (n + 16 * WMSE_THREADS - 1) / (16 * WMSE_THREADS);
    if (s > WMSE_MAX_BLOCKS) s = WMSE_MAX_BLOCKS;
    return s < 1 ? 1 : (int)s;
}

// one element: the sum takes the difference in float64 (exact for fp32 operands), the map the fp32 difference times g2 = 2 gscale
__device__ __forceinline__ float wmse_elem(float o, float t, const wmse_gate& g, float g2, double& sum, unsigned& cnt) {
    const bool in = ((o - g.omin) > g.otho) & ((t - g.tmin) > g.ttho);
    const double dd = (double)o - (double)t;
    sum += in ? dd * dd : 0.0;
    cnt += in ? 1u : 0u;
    return in ? g2 * (o - t) : 0.f;
}

// Block b works on elements [b * per, min(n, (b + 1) * per)), per a multiple of four: the slices start on 16-byte boundaries where the
// tensors do.  `vec`: output, target and grad are 16-byte aligned; the body then moves on 16-byte accesses, WMSE_UNROLL loads per
// tensor in flight per thread, and the ragged end of the slice element by element.
template <bool GRAD>
__global__ __launch_bounds__(WMSE_THREADS) void wmse_kernel(const float* __restrict__ output, const float* __restrict__ target,
                                                            const float* __restrict__ extrema, float ths_perc, float g2,
                                                            float* __restrict__ grad, double* __restrict__ slab, int64_t n, int vec) {
    __shared__ double red[16];
    wmse_gate g;
    g.omin = extrema[0];
    g.otho = (extrema[1] - g.omin) * ths_perc;
    g.tmin = extrema[4];
    g.ttho = (extrema[5] - g.tmin) * ths_perc;
    const int64_t per = (((n + gridDim.x - 1) / gridDim.x) + 3) & ~(int64_t)3;
    const int64_t lo = (int64_t)blockIdx.x * per < n ? (int64_t)blockIdx.x * per : n, hi = lo + per < n ? lo + per : n;
    const int64_t bd = WMSE_THREADS;
    double sum = 0.0;
    unsigned cnt = 0;                                             // a thread sees n / 2^19 elements at the most
    int64_t done = lo;
    if (vec) {
        const int64_t n4 = (hi - lo) >> 2;
        const f32x4* o4 = reinterpret_cast<const f32x4*>(output + lo);
        const f32x4* t4 = reinterpret_cast<const f32x4*>(target + lo);
        f32x4* g4 = GRAD ? reinterpret_cast<f32x4*>(grad + lo) : nullptr;
        int64_t i = threadIdx.x;
        for (; i + (WMSE_UNROLL - 1) * bd < n4; i += WMSE_UNROLL * bd) {
            f32x4 vo[WMSE_UNROLL], vt[WMSE_UNROLL];
#pragma unroll
            for (int u = 0; u < WMSE_UNROLL; ++u) {
                vo[u] = o4[i + u * bd];
                vt[u] = t4[i + u * bd];
            }
#pragma unroll
            for (int u = 0; u < WMSE_UNROLL; ++u) {
                f32x4 r;
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = wmse_elem(vo[u][j], vt[u][j], g, g2, sum, cnt);
                if constexpr (GRAD) g4[i + u * bd] = r;
            }
        }
        for (; i < n4; i += bd) {
            const f32x4 vo = o4[i], vt = t4[i];
            f32x4 r;
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = wmse_elem(vo[j], vt[j], g, g2, sum, cnt);
            if constexpr (GRAD) g4[i] = r;
        }
        done = lo + (n4 << 2);
    }
    for (int64_t i = done + threadIdx.x; i < hi; i += bd) {
        const float r = wmse_elem(output[i], target[i], g, g2, sum, cnt);
        if constexpr (GRAD) grad[i] = r;
    }
    sum = cwfa_block_sum(sum, red);
    const double c = cwfa_block_sum((double)cnt, red);          // integers below 2^53: exact
    if (threadIdx.x == 0) {
        slab[2 * (int64_t)blockIdx.x] = sum;
        slab[2 * (int64_t)blockIdx.x + 1] = c;
    }
}

// out[2] = the slab's two columns, each thread its rows in ascending order, then the block sum: one fixed order
__global__ __launch_bounds__(WMSE_THREADS) void wmse_finish_kernel(const double* __restrict__ slab, int blocks, double* __restrict__ out) {
    __shared__ double red[16];
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < blocks; i += WMSE_THREADS) {
        acc[0] += slab[2 * i];
        acc[1] += slab[2 * i + 1];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double r = cwfa_block_sum(acc[k], red);
        if (threadIdx.x == 0) out[k] = r;
    }
}

extern "C" int64_t cwfa_wmse_workspace_bytes(int64_t n) {
    CWFA_REQUIRE(n >= 0, CWFA_E_INVAL, "cwfa_wmse_workspace_bytes: negative size");
    return n == 0 ? 0 : (int64_t)wmse_blocks(n) * 2 * (int64_t)sizeof(double);
}

extern "C" int cwfa_wmse_loss_f32(const float* output, const float* target, const float* extrema, float ths_perc, float gscale,
                                  float* grad, double* out, void* workspace, int64_t n, void* stream) {
    CWFA_REQUIRE(out != nullptr, CWFA_E_INVAL, "cwfa_wmse_loss_f32: null out");
    CWFA_REQUIRE(n >= 0, CWFA_E_INVAL, "cwfa_wmse_loss_f32: negative n");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(out, 0, 2 * sizeof(double), st) != hipSuccess) {
            cwfa_set_error("cwfa_wmse_loss_f32: clearing out failed");
            return CWFA_E_HIP;
        }
        return CWFA_OK;
    }
    CWFA_REQUIRE(output && target && extrema && workspace, CWFA_E_INVAL, "cwfa_wmse_loss_f32: null pointer");
    CWFA_REQUIRE((((uintptr_t)output | (uintptr_t)target | (uintptr_t)grad | (uintptr_t)extrema) & 3u) == 0 &&
                     (((uintptr_t)out | (uintptr_t)workspace) & 7u) == 0,
                 CWFA_E_ALIGN, "cwfa_wmse_loss_f32: a float pointer is not 4-byte, or a double pointer not 8-byte aligned");
    const int blocks = wmse_blocks(n);
    const float g2 = 2.0f * gscale;
    double* slab = static_cast<double*>(workspace);
    if (grad) {
        const int vec = cwfa_aligned16(output) && cwfa_aligned16(target) && cwfa_aligned16(grad);
        hipLaunchKernelGGL(wmse_kernel<true>, dim3(blocks), dim3(WMSE_THREADS), 0, st, output, target, extrema, ths_perc, g2, grad, slab, n,
                           vec);
    } else {
        const int vec = cwfa_aligned16(output) && cwfa_aligned16(target);
        hipLaunchKernelGGL(wmse_kernel<false>, dim3(blocks), dim3(WMSE_THREADS), 0, st, output, target, extrema, ths_perc, g2, grad, slab,
                           n, vec);
    }
    CWFA_LAUNCH_CHECK("cwfa_wmse_loss_f32");
    hipLaunchKernelGGL(wmse_finish_kernel, dim3(1), dim3(WMSE_THREADS), 0, st, slab, blocks, out);
    CWFA_LAUNCH_CHECK("cwfa_wmse_loss_f32");
    return CWFA_OK;
}
