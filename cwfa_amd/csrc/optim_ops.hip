// The parameter update behind `scaler.step(optimizer)` / `optimizer.step()` (reference CWFA.py:1011-1027): the Lion rule with
// decoupled weight decay over MANY fp32 tensors in one launch, the GradScaler's unscale and skip-on-inf decided on the device.
// A streaming kernel: 12 bytes read and 8 written per element.  Built with -ffp-contract=off: every fp32 operation is rounded
// separately (at most four roundings per output).
#include "common.h"

#define LION_THREADS 256
#define LION_VECS (CWFA_LION_BLOCK_ELEMS / (4 * LION_THREADS))      // 16-byte groups per thread of a full block
static_assert(CWFA_LION_BLOCK_ELEMS == 4 * LION_THREADS * LION_VECS, "a block is a whole number of 16-byte groups per thread");

// The kernel's argument: the tensors that have elements, and for each the first block that works on it (ascending; a block
// finds its tensor by bisection).  It travels in the kernel-argument segment (4 KiB with the scalars and the hidden arguments).
struct lion_args {
    cwfa_lion_tensor t[CWFA_LION_MAX_TENSORS];
    int first_block[CWFA_LION_MAX_TENSORS];
    int n;
};
static_assert(sizeof(lion_args) <= 3584, "lion_args must leave room for the scalars and the hidden kernel arguments");

struct lion_hyper {
    float lr, beta1, omb1, beta2, omb2, decay;      // omb = fp32(1) - beta, decay = fp32(1) - fp32(lr * wd)
};

// p <- p * decay;  u = sign(beta1 * m + omb1 * g);  p <- p - lr * u;  m <- beta2 * m + omb2 * g      (g already unscaled)
__device__ __forceinline__ void lion_update(float& p, float& m, float g, const lion_hyper& h) {
    const float c = h.beta1 * m + h.omb1 * g;
    const float u = (float)((c > 0.f) - (c < 0.f));              // sign(0) = 0; NaN compares false both ways
    p = p * h.decay - h.lr * u;
    m = h.beta2 * m + h.omb2 * g;
}

__global__ __launch_bounds__(LION_THREADS) void lion_step_kernel(lion_args a, lion_hyper h, const float* __restrict__ grad_scale,
                                                                 const float* __restrict__ found_inf) {
    if (found_inf != nullptr && *found_inf != 0.f) return;       // the scaler saw inf / NaN: nothing is written
    const bool scaled = grad_scale != nullptr;
    const float scale = scaled ? *grad_scale : 1.f;
    const int b = blockIdx.x;
    int lo = 0, hi = a.n;                                         // the last tensor whose first block is <= b
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first_block[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    const cwfa_lion_tensor t = a.t[lo];
    const int64_t off = (int64_t)(b - a.first_block[lo]) * CWFA_LION_BLOCK_ELEMS;
    const int64_t left = t.numel - off;
    const int cnt = left < CWFA_LION_BLOCK_ELEMS ? (int)left : CWFA_LION_BLOCK_ELEMS;
    float* __restrict__ p = t.p + off;
    const float* __restrict__ g = t.g + off;
    float* __restrict__ m = t.m + off;
    const int tid = threadIdx.x;
    int done = 0;
    // off is a multiple of four elements: the block is 16-byte aligned where the three tensors are
    if (((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m)) & 15u) == 0) {
        f32x4* p4 = reinterpret_cast<f32x4*>(p);
        const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
        f32x4* m4 = reinterpret_cast<f32x4*>(m);
        const int n4 = cnt >> 2;
        if (n4 == LION_THREADS * LION_VECS) {                     // a full block: every load in flight before the first use
            f32x4 pv[LION_VECS], gv[LION_VECS], mv[LION_VECS];
#pragma unroll
            for (int u = 0; u < LION_VECS; ++u) {
                pv[u] = p4[tid + u * LION_THREADS];
                gv[u] = g4[tid + u * LION_THREADS];
                mv[u] = m4[tid + u * LION_THREADS];
            }
#pragma unroll
            for (int u = 0; u < LION_VECS; ++u) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pe = pv[u][j], me = mv[u][j];
                    lion_update(pe, me, scaled ? gv[u][j] / scale : gv[u][j], h);
                    pv[u][j] = pe;
                    mv[u][j] = me;
                }
                p4[tid + u * LION_THREADS] = pv[u];
                m4[tid + u * LION_THREADS] = mv[u];
            }
        } else {
            for (int i = tid; i < n4; i += LION_THREADS) {
                f32x4 pv = p4[i], mv = m4[i];
                const f32x4 gv = g4[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pe = pv[j], me = mv[j];
                    lion_update(pe, me, scaled ? gv[j] / scale : gv[j], h);
                    pv[j] = pe;
                    mv[j] = me;
                }
                p4[i] = pv;
                m4[i] = mv;
            }
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < cnt; i += LION_THREADS) {      // unaligned tensors and ragged ends
        float pe = p[i], me = m[i];
        lion_update(pe, me, scaled ? g[i] / scale : g[i], h);
        p[i] = pe;
        m[i] = me;
    }
}

extern "C" int cwfa_lion_step_f32(const cwfa_lion_table* tab, float lr, float beta1, float beta2, float weight_decay,
                                  const float* grad_scale, const float* found_inf, void* stream) {
    CWFA_REQUIRE(tab != nullptr, CWFA_E_INVAL, "cwfa_lion_step_f32: null table");
    CWFA_REQUIRE(tab->n >= 0 && tab->n <= CWFA_LION_MAX_TENSORS, CWFA_E_INVAL, "cwfa_lion_step_f32: n = %d is not in 0 .. %d", tab->n,
                 CWFA_LION_MAX_TENSORS);
    lion_args a;
    a.n = 0;
    int64_t blocks = 0;
    for (int i = 0; i < tab->n; ++i) {
        const cwfa_lion_tensor& t = tab->t[i];
        CWFA_REQUIRE(t.numel >= 0, CWFA_E_INVAL, "cwfa_lion_step_f32: tensor %d has a negative size", i);
        CWFA_REQUIRE(t.numel < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_lion_step_f32: tensor %d has 2^31 or more elements", i);
        if (t.numel == 0) continue;
        CWFA_REQUIRE(t.p != nullptr && t.g != nullptr && t.m != nullptr, CWFA_E_INVAL, "cwfa_lion_step_f32: tensor %d has a null pointer", i);
        CWFA_REQUIRE((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m) & 3u) == 0, CWFA_E_ALIGN,
                     "cwfa_lion_step_f32: tensor %d is not 4-byte aligned", i);
        a.t[a.n] = t;
        a.first_block[a.n] = (int)blocks;
        ++a.n;
        blocks += (t.numel + CWFA_LION_BLOCK_ELEMS - 1) / CWFA_LION_BLOCK_ELEMS;
        CWFA_REQUIRE(blocks <= 0x7fffffff, CWFA_E_SHAPE, "cwfa_lion_step_f32: more blocks than a grid holds");
    }
    if (a.n == 0) return CWFA_OK;
    for (int i = a.n; i < CWFA_LION_MAX_TENSORS; ++i) {          // the unused tail is copied with the argument: keep it defined
        a.t[i] = cwfa_lion_tensor{nullptr, nullptr, nullptr, 0};
        a.first_block[i] = 0x7fffffff;
    }
    lion_hyper h;
    h.lr = lr;
    h.beta1 = beta1;
    h.omb1 = 1.0f - beta1;
    h.beta2 = beta2;
    h.omb2 = 1.0f - beta2;
    h.decay = 1.0f - lr * weight_decay;
    hipLaunchKernelGGL(lion_step_kernel, dim3((unsigned)blocks), dim3(LION_THREADS), 0, (hipStream_t)stream, a, h, grad_scale, found_inf);
    CWFA_LAUNCH_CHECK("cwfa_lion_step_f32");
    return CWFA_OK;
}
