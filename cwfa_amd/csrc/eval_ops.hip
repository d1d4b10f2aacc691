// The evaluation pass behind a reconstructed volume (reference CWFA.py:1032-1117): extrema, PSNR / masked-MAE sums, the three
// maximum projections and their composite image, ROI traces and the median of the positives.  All HBM-bound streaming kernels
// over fp32 [B, D, H, W] tensors.  Inputs are assumed finite: NaN propagation is not provided.
#include <math.h>
#include "common.h"

// the optional de-normalisation on load, v -> (v * 2^-step) * std - mean, as two separately rounded fp32 operations after the
// exact power-of-two scaling (the library is built with -ffp-contract=off): the bits of CWFA.py:112-113,116-117
struct EvalAff {
    int on;
    float sc, sd, mn;
};
static inline EvalAff eval_aff(const cwfa_eval_affine* a) {
    EvalAff r = {0, 1.f, 1.f, 0.f};
    if (a && a->enabled) r = {1, a->scale, a->std, a->mean};
    return r;
}
__device__ __forceinline__ float eval_load(float v, const EvalAff& a) { return a.on ? (v * a.sc) * a.sd - a.mn : v; }

__device__ __forceinline__ unsigned f2u(float v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ float u2f(unsigned v) { return __builtin_bit_cast(float, v); }

// Stream the block's slice of one sample: f(a_i, b_i) for every element (b_i = 0 without a second tensor).  The slices start on
// 16-byte boundaries; `vec`: both sample bases are 16-byte aligned, so the body runs on 16-byte loads, four (eight with two
// tensors) in flight per thread, and the ragged end of the sample on scalar loads.
template <bool TWO, class F>
__device__ __forceinline__ void eval_stream(const float* __restrict__ pa, const float* __restrict__ pb, int64_t n, int vec, F&& f) {
    const int64_t per = (((n + gridDim.x - 1) / gridDim.x) + 3) & ~(int64_t)3;
    const int64_t lo = (int64_t)blockIdx.x * per < n ? (int64_t)blockIdx.x * per : n, hi = lo + per < n ? lo + per : n;
    const int64_t bd = blockDim.x;
    int64_t done = lo;
    if (vec) {
        const int64_t n4 = (hi - lo) >> 2;
        const f32x4* a4 = reinterpret_cast<const f32x4*>(pa + lo);
        const f32x4* b4 = TWO ? reinterpret_cast<const f32x4*>(pb + lo) : nullptr;
        int64_t i = threadIdx.x;
        for (; i + 3 * bd < n4; i += 4 * bd) {
            f32x4 va[4], vb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                va[u] = a4[i + u * bd];
                if constexpr (TWO) vb[u] = b4[i + u * bd];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) f(va[u][j], TWO ? vb[u][j] : 0.f);
        }
        for (; i < n4; i += bd) {
            const f32x4 va = a4[i];
            f32x4 vb = {0.f, 0.f, 0.f, 0.f};
            if constexpr (TWO) vb = b4[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) f(va[j], vb[j]);
        }
        done = lo + (n4 << 2);
    }
    for (int64_t i = done + threadIdx.x; i < hi; i += bd) f(pa[i], TWO ? pb[i] : 0.f);
}

// blocks per sample of the streaming kernels: the chip several times over, >= 4096 elements per block, a fixed function of the
// shape (the float64 partial sums are added in a fixed order: results are bitwise reproducible)
static inline int eval_splits(int64_t n, int B) {
    int64_t s = (n + 256 * 16 - 1) / (256 * 16), want = (2048 + B - 1) / B;
    if (s > want) s = want;
    if (s > CWFA_EVAL_MAX_SPLITS) s = CWFA_EVAL_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}
// 16-byte loads: every sample base is 16-byte aligned (the batch stride counts only where there is a second sample)
static inline int eval_vec(int B, const float* a, int64_t a_bs, const float* b, int64_t b_bs) {
    return cwfa_aligned16(a) && (B <= 1 || (a_bs & 3) == 0) && (!b || (cwfa_aligned16(b) && (B <= 1 || (b_bs & 3) == 0)));
}

extern "C" int64_t cwfa_eval_splits(int B, int64_t n) {
    CWFA_REQUIRE(B >= 0 && n >= 0, CWFA_E_INVAL, "cwfa_eval_splits: negative size");
    return (B == 0 || n == 0) ? 0 : eval_splits(n, B);
}

// block-wide maximum (blockDim.x multiple of 64, <= 1024), result valid in thread 0
__device__ __forceinline__ float eval_block_max(float v, float* lds /* >= 16 floats */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    float r = v;
    if (threadIdx.x == 0)
        for (int i = 0; i < nw; ++i) r = fmaxf(r, lds[i]);
    __syncthreads();
    return r;
}

// ------------------------------------------------------------------------------------------------ extrema
// Per block the ten maxima of its slice (minima as maxima of the negated values) go to a slab [B][splits][10]; the finish kernel
// takes the maximum over the slab.  (Atomics on the ten result words serialise: 2048 blocks x 10 took 0.2 ms at 512 x 512 x 96.)
template <bool TWO>
__global__ __launch_bounds__(256) void extrema_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n, int64_t a_bs,
                                                      int64_t b_bs, EvalAff af, float* __restrict__ slab, int vec) {
    __shared__ float red[16];
    const int s = blockIdx.y;
    // m[k]: -min a, max a, -min|a|, max|a|, the same four of b, -min|a-b|, max|a-b|
    float m[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) m[k] = -INFINITY;
    eval_stream<TWO>(a + s * a_bs, TWO ? b + s * b_bs : nullptr, n, vec, [&](float va, float vb) {
        const float x = eval_load(va, af), ax = fabsf(x);
        m[0] = fmaxf(m[0], -x), m[1] = fmaxf(m[1], x), m[2] = fmaxf(m[2], -ax), m[3] = fmaxf(m[3], ax);
        if constexpr (TWO) {
            const float y = eval_load(vb, af), ay = fabsf(y), dd = fabsf(x - y);
            m[4] = fmaxf(m[4], -y), m[5] = fmaxf(m[5], y), m[6] = fmaxf(m[6], -ay), m[7] = fmaxf(m[7], ay);
            m[8] = fmaxf(m[8], -dd), m[9] = fmaxf(m[9], dd);
        }
    });
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const float r = eval_block_max(m[k], red);
        if (threadIdx.x == 0) slab[((int64_t)s * gridDim.x + blockIdx.x) * 10 + k] = r;
    }
}

__global__ __launch_bounds__(256) void extrema_finish_kernel(const float* __restrict__ slab, int splits, int nvals, float* __restrict__ out) {
    __shared__ float red[16];
    const int s = blockIdx.x;
    float m[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) m[k] = -INFINITY;
    for (int i = threadIdx.x; i < splits; i += blockDim.x)
#pragma unroll
        for (int k = 0; k < 10; ++k) m[k] = fmaxf(m[k], slab[((int64_t)s * splits + i) * 10 + k]);
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const float r = eval_block_max(m[k], red);
        if (threadIdx.x == 0) out[s * CWFA_EXTREMA_STRIDE + k] = k < nvals ? ((k & 1) ? r : -r) : 0.f;
    }
    if (threadIdx.x == 0) out[s * CWFA_EXTREMA_STRIDE + 10] = out[s * CWFA_EXTREMA_STRIDE + 11] = 0.f;
}

extern "C" int cwfa_volume_extrema_f32(const float* a, const float* b, float* out, float* workspace, int B, int64_t n, int64_t a_bs,
                                       int64_t b_bs, const cwfa_eval_affine* affine, void* stream) {
    CWFA_REQUIRE(a && out && workspace, CWFA_E_INVAL, "cwfa_volume_extrema_f32: null pointer");
    CWFA_REQUIRE(B >= 0 && n >= 0 && B <= 65535, CWFA_E_SHAPE, "cwfa_volume_extrema_f32: bad shape");
    CWFA_REQUIRE(a_bs >= 0 && b_bs >= 0 && (B <= 1 || (a_bs >= n && (!b || b_bs >= n))), CWFA_E_INVAL,
                 "cwfa_volume_extrema_f32: batch stride smaller than a sample");
    if (B == 0 || n == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    const EvalAff af = eval_aff(affine);
    const int splits = eval_splits(n, B);
    const dim3 grid(splits, B);
    const int vec = eval_vec(B, a, a_bs, b, b_bs);
    if (b)
        hipLaunchKernelGGL(extrema_kernel<true>, grid, dim3(256), 0, st, a, b, n, a_bs, b_bs, af, workspace, vec);
    else
        hipLaunchKernelGGL(extrema_kernel<false>, grid, dim3(256), 0, st, a, b, n, a_bs, b_bs, af, workspace, vec);
    CWFA_LAUNCH_CHECK("cwfa_volume_extrema_f32");
    hipLaunchKernelGGL(extrema_finish_kernel, dim3(B), dim3(256), 0, st, workspace, splits, b ? 10 : 4, out);
    CWFA_LAUNCH_CHECK("cwfa_volume_extrema_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ PSNR / masked-MAE sums
// Per block the four float64 sums of its slice go to a slab [B][splits][4]; the finish kernel adds the slab in a fixed order.
// The differences are formed in float64 (exact for fp32 operands), the squares are rounded once.
__global__ __launch_bounds__(256) void metrics_kernel(const float* __restrict__ p, const float* __restrict__ g, int64_t n, int64_t p_bs,
                                                      int64_t g_bs, EvalAff af, float p_off, float g_off, float thr,
                                                      double* __restrict__ slab, int vec) {
    __shared__ double red[16];
    const int s = blockIdx.y;
    double sse = 0.0, sg = 0.0, sam = 0.0, cnt = 0.0;
    eval_stream<true>(p + s * p_bs, g + s * g_bs, n, vec, [&](float vp, float vg) {
        const float x = eval_load(vp, af) - p_off, y = eval_load(vg, af) - g_off;
        const double dd = (double)y - (double)x;
        sse += dd * dd;
        sg += (double)y;
        const bool masked = x < thr;
        sam += fabs((double)y - (masked ? 0.0 : (double)x));
        cnt += masked ? 1.0 : 0.0;
    });
    sse = cwfa_block_sum(sse, red);
    sg = cwfa_block_sum(sg, red);
    sam = cwfa_block_sum(sam, red);
    cnt = cwfa_block_sum(cnt, red);
    if (threadIdx.x == 0) {
        double* o = slab + ((int64_t)s * gridDim.x + blockIdx.x) * 4;
        o[0] = sse, o[1] = sg, o[2] = sam, o[3] = cnt;
    }
}

__global__ __launch_bounds__(256) void metrics_finish_kernel(const double* __restrict__ slab, int splits, double* __restrict__ out) {
    __shared__ double red[16];
    const int s = blockIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < splits; i += blockDim.x)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += slab[((int64_t)s * splits + i) * 4 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double r = cwfa_block_sum(acc[k], red);
        if (threadIdx.x == 0) out[s * 4 + k] = r;
    }
}

extern "C" int cwfa_volume_metrics_f32(const float* pred, const float* gt, double* out, double* workspace, int B, int64_t n,
                                       int64_t pred_bs, int64_t gt_bs, const cwfa_eval_affine* affine, float pred_offset,
                                       float gt_offset, float thr, void* stream) {
    CWFA_REQUIRE(pred && gt && out && workspace, CWFA_E_INVAL, "cwfa_volume_metrics_f32: null pointer");
    CWFA_REQUIRE(B >= 0 && n >= 0 && B <= 65535, CWFA_E_SHAPE, "cwfa_volume_metrics_f32: bad shape");
    CWFA_REQUIRE(pred_bs >= 0 && gt_bs >= 0 && (B <= 1 || (pred_bs >= n && gt_bs >= n)), CWFA_E_INVAL,
                 "cwfa_volume_metrics_f32: batch stride smaller than a sample");
    if (B == 0 || n == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    const int splits = eval_splits(n, B);
    hipLaunchKernelGGL(metrics_kernel, dim3(splits, B), dim3(256), 0, st, pred, gt, n, pred_bs, gt_bs, eval_aff(affine), pred_offset,
                       gt_offset, thr, workspace, eval_vec(B, pred, pred_bs, gt, gt_bs));
    CWFA_LAUNCH_CHECK("cwfa_volume_metrics_f32");
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(B), dim3(256), 0, st, workspace, splits, out);
    CWFA_LAUNCH_CHECK("cwfa_volume_metrics_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ maximum projections
// The maps volume_2_projections applies to the volume before it projects (utils.py:293-303), here applied on load:
// normalise ((v - sub) / div), lower threshold to zero, upper clamp to a constant -- in fp32 and in the reference's order.
struct EvalPost {
    int normalize, thresh;
    float nsub, ndiv, tmin, tlo, thi, tval;
};
__device__ __forceinline__ float eval_post(float v, const EvalPost& q) {
    if (q.normalize) v = (v - q.nsub) / q.ndiv;
    if (q.thresh) {
        if ((v - q.tmin) < q.tlo) v = 0.f;
        if ((v - q.tmin) > q.thi) v = q.tval;
    }
    return v;
}

// "mip3_ablate" option (measurement only, the results are then wrong): bit 0 drops the stores of the over-depth image, bit 1 the
// LDS maxima and stores of the over-H image, bit 2 the wave reductions and stores of the over-W image
int g_cwfa_mip3_ablate = 0;

#define MIP_TW 256   // columns of a block's tile: one 16-byte load per lane covers a 1 KiB row segment per wave
#define MIP_R 4      // rows per wave
#define MIP_TH 16    // rows of the tile (4 waves)
#define MIP_DC 8     // most depths of a block's chunk (the LDS images of the two small projections)

// NP = 1: the projections of |a| (or of |a - b| with a second tensor); NP = 3: those of |a|, |b| and |a - b| in the same read.
// A block owns a 16 x 256 tile of the plane over a chunk of depths.  The maximum over depth stays in registers; the maximum over
// H is collected per depth in LDS (the four waves hold different rows of the same columns: LDS integer maxima), the maximum
// over W is a wave reduction per row.  At the end the three images go out with integer atomic maxima: the values are
// non-negative, so their bit patterns order like unsigned integers, the results are exact and independent of the order.
template <int NP>
__global__ __launch_bounds__(256) void mip3_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t a_bs, int64_t b_bs,
                                                   EvalAff af, EvalPost post, unsigned* __restrict__ zp, unsigned* __restrict__ xp,
                                                   unsigned* __restrict__ yp, unsigned* __restrict__ gmin, int B, int D, int H, int W,
                                                   int dchunk, int nchunks, int vec, int ablate) {
    __shared__ unsigned xs[NP * MIP_DC * MIP_TW];
    __shared__ unsigned ys[NP * MIP_DC * MIP_TH];
    __shared__ float red[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.z / nchunks, ch = blockIdx.z % nchunks;
    const int d0 = ch * dchunk, d1 = d0 + dchunk < D ? d0 + dchunk : D;
    const int w0 = blockIdx.x * MIP_TW + lane * 4, h0 = blockIdx.y * MIP_TH + wave * MIP_R;
    const float* pa = a + s * a_bs;
    const float* pb = b ? b + s * b_bs : nullptr;
    const bool diff = NP == 1 && b != nullptr;
    for (int i = threadIdx.x; i < NP * MIP_DC * MIP_TW; i += 256) xs[i] = 0;
    for (int i = threadIdx.x; i < NP * MIP_DC * MIP_TH; i += 256) ys[i] = 0;
    __syncthreads();

    float zmax[NP][MIP_R][4], mn[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        mn[q] = INFINITY;
#pragma unroll
        for (int r = 0; r < MIP_R; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) zmax[q][r][c] = 0.f;
    }
    for (int d = d0; d < d1; ++d) {
        const int j = d - d0;
        f32x4 va[MIP_R], vb[MIP_R];
#pragma unroll
        for (int r = 0; r < MIP_R; ++r) {
            va[r] = vb[r] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int h = h0 + r;
            if (h < H && w0 < W) {
                const int64_t o = ((int64_t)d * H + h) * W + w0;
                if (vec) {
                    va[r] = *reinterpret_cast<const f32x4*>(pa + o);
                    if (pb) vb[r] = *reinterpret_cast<const f32x4*>(pb + o);
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (w0 + c < W) {
                            va[r][c] = pa[o + c];
                            if (pb) vb[r][c] = pb[o + c];
                        }
                }
            }
        }
        float xm[NP][4];
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) xm[q][c] = 0.f;
#pragma unroll
        for (int r = 0; r < MIP_R; ++r) {
            const int h = h0 + r;
            if (h >= H) continue;                                   // wave-uniform
            float rm[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) rm[q] = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool ok = w0 + c < W;
                const float x = eval_load(va[r][c], af), y = eval_load(vb[r][c], af);
                float v[NP];
                if constexpr (NP == 1) {
                    v[0] = eval_post(diff ? fabsf(x - y) : fabsf(x), post);
                } else {
                    v[0] = fabsf(x), v[1] = fabsf(y), v[2] = fabsf(x - y);
                }
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const float vm = ok ? v[q] : 0.f;
                    zmax[q][r][c] = fmaxf(zmax[q][r][c], vm);
                    xm[q][c] = fmaxf(xm[q][c], vm);
                    rm[q] = fmaxf(rm[q], vm);
                    mn[q] = fminf(mn[q], ok ? v[q] : INFINITY);
                }
            }
            if (ablate & 4) continue;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                float m = rm[q];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
                if (lane == 0) ys[(q * MIP_DC + j) * MIP_TH + wave * MIP_R + r] = f2u(m);
            }
        }
        // column c of lane l sits at c * 64 + l: consecutive lanes, consecutive banks
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (!(ablate & 2)) atomicMax(&xs[(q * MIP_DC + j) * MIP_TW + c * 64 + lane], f2u(xm[q][c]));
    }
    __syncthreads();

    const int nd = d1 - d0;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int64_t img = (int64_t)q * B + s;
        // over depth -> [H, W]
#pragma unroll
        for (int r = 0; r < MIP_R; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (h0 + r < H && w0 + c < W && !(ablate & 1)) {
                    unsigned* dst = &zp[(img * H + h0 + r) * W + w0 + c];
                    if (nchunks == 1)
                        *dst = f2u(zmax[q][r][c]);
                    else
                        atomicMax(dst, f2u(zmax[q][r][c]));
                }
        // over H -> [W, D]: consecutive threads, consecutive depths of one column
        for (int i = threadIdx.x; i < MIP_TW * nd && !(ablate & 2); i += 256) {
            const int wl = i / nd, jj = i % nd, w = blockIdx.x * MIP_TW + wl;
            if (w < W) atomicMax(&xp[(img * W + w) * D + d0 + jj], xs[(q * MIP_DC + jj) * MIP_TW + (wl & 3) * 64 + (wl >> 2)]);
        }
        // over W -> [H, D]
        for (int i = threadIdx.x; i < MIP_TH * nd && !(ablate & 4); i += 256) {
            const int hl = i / nd, jj = i % nd, h = blockIdx.y * MIP_TH + hl;
            if (h < H) atomicMax(&yp[(img * H + h) * D + d0 + jj], ys[(q * MIP_DC + jj) * MIP_TH + hl]);
        }
        const float m = -eval_block_max(-mn[q], red);
        if (threadIdx.x == 0) atomicMin(&gmin[img], f2u(m));
    }
}

extern "C" int cwfa_mip3_f32(const float* a, const float* b, float* zproj, float* xproj, float* yproj, float* gmin, int B, int D,
                             int H, int W, int64_t a_bs, int64_t b_bs, int triple, const cwfa_eval_affine* affine,
                             const cwfa_eval_post* post, void* stream) {
    CWFA_REQUIRE(a && zproj && xproj && yproj && gmin, CWFA_E_INVAL, "cwfa_mip3_f32: null pointer");
    CWFA_REQUIRE(!triple || b, CWFA_E_INVAL, "cwfa_mip3_f32: the three-image form needs both tensors");
    CWFA_REQUIRE(!triple || !post, CWFA_E_INVAL, "cwfa_mip3_f32: the volume maps go with the one-image form only");
    CWFA_REQUIRE(B >= 0 && D >= 0 && H >= 0 && W >= 0, CWFA_E_SHAPE, "cwfa_mip3_f32: negative size");
    const int64_t n = (int64_t)D * H * W;
    CWFA_REQUIRE(a_bs >= 0 && b_bs >= 0 && (B <= 1 || (a_bs >= n && (!b || b_bs >= n))), CWFA_E_INVAL,
                 "cwfa_mip3_f32: batch stride smaller than a sample");
    if (B == 0 || n == 0) return CWFA_OK;
    const int tx = (W + MIP_TW - 1) / MIP_TW, ty = (H + MIP_TH - 1) / MIP_TH;
    // chunks of at most MIP_DC depths, more of them while the grid is short of ~1024 blocks
    int nchunks = (D + MIP_DC - 1) / MIP_DC;
    const int64_t want = (1024 + (int64_t)tx * ty * B - 1) / ((int64_t)tx * ty * B);
    if (nchunks < want) nchunks = want < D ? (int)want : D;
    const int dchunk = (D + nchunks - 1) / nchunks;
    nchunks = (D + dchunk - 1) / dchunk;
    CWFA_REQUIRE(ty <= 65535 && (int64_t)B * nchunks <= 65535, CWFA_E_SHAPE, "cwfa_mip3_f32: grid too large");
    hipStream_t st = (hipStream_t)stream;
    const int np = triple ? 3 : 1;
    hipError_t e = hipMemsetAsync(zproj, 0, sizeof(float) * np * B * H * W, st);
    if (e == hipSuccess) e = hipMemsetAsync(xproj, 0, sizeof(float) * np * B * W * D, st);
    if (e == hipSuccess) e = hipMemsetAsync(yproj, 0, sizeof(float) * np * B * H * D, st);
    if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(gmin), 0x7f800000, np * B, st);
    if (e != hipSuccess) {
        cwfa_set_error("cwfa_mip3_f32: clearing the outputs failed: %s", hipGetErrorString(e));
        return CWFA_E_HIP;
    }
    EvalPost q = {0, 0, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f};
    if (post) q = {post->normalize, post->threshold, post->norm_sub, post->norm_div, post->vol_min, post->lower, post->upper, post->clamp_value};
    const int vec = (W & 3) == 0 && eval_vec(B, a, a_bs, b, b_bs);
    const dim3 grid(tx, ty, B * nchunks);
    unsigned *z = reinterpret_cast<unsigned*>(zproj), *x = reinterpret_cast<unsigned*>(xproj), *y = reinterpret_cast<unsigned*>(yproj),
             *g = reinterpret_cast<unsigned*>(gmin);
    if (triple)
        hipLaunchKernelGGL(mip3_kernel<3>, grid, dim3(256), 0, st, a, b, a_bs, b_bs, eval_aff(affine), q, z, x, y, g, B, D, H, W, dchunk, nchunks, vec, g_cwfa_mip3_ablate);
    else
        hipLaunchKernelGGL(mip3_kernel<1>, grid, dim3(256), 0, st, a, b, a_bs, b_bs, eval_aff(affine), q, z, x, y, g, B, D, H, W, dchunk, nchunks, vec, g_cwfa_mip3_ablate);
    CWFA_LAUNCH_CHECK("cwfa_mip3_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ composite image
// utils.py:305-325 on the three projections of a [D, H, W] volume (H == W, the plane unscaled): the over-depth image top left,
// the over-H image transposed to [D*sf, W] below it, the over-W image [H, D*sf] to its right, nearest-neighbour replication
// along depth by ATen's rule src = min(floor(dst * fp32(in / out)), in - 1), the rest filled, scale-bar lines of 1.0 on top.
__global__ __launch_bounds__(256) void compose_kernel(const float* __restrict__ zp, const float* __restrict__ xp, const float* __restrict__ yp,
                                                      const float* __restrict__ fill, float* __restrict__ out, int D, int H, int W,
                                                      int s4, int bt, int bars, float dscale) {
    const int OH = H + s4 + bt, OW = W + s4 + bt;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)OH * OW) return;
    const int s = blockIdx.y, r = (int)(i / OW), c = (int)(i % OW);
    float v = *fill;
    if (r < H && c < W) {
        v = zp[((int64_t)s * H + r) * W + c];
    } else if (r >= H + bt && c < W) {
        int sd = (int)floorf((float)(r - H - bt) * dscale);
        sd = sd < D - 1 ? sd : D - 1;
        v = xp[((int64_t)s * W + c) * D + sd];
    } else if (r < H && c >= W + bt) {
        int sd = (int)floorf((float)(c - W - bt) * dscale);
        sd = sd < D - 1 ? sd : D - 1;
        v = yp[((int64_t)s * H + r) * D + sd];
    }
    if (bars && ((r >= H && r < H + bt) || (c >= W && c < W + bt))) v = 1.0f;
    out[(int64_t)s * OH * OW + i] = v;
}

extern "C" int cwfa_projection_compose_f32(const float* zproj, const float* xproj, const float* yproj, const float* fill, float* out,
                                           int B, int D, int H, int W, int depth_scale, int border, int scale_bars, void* stream) {
    CWFA_REQUIRE(zproj && xproj && yproj && fill && out, CWFA_E_INVAL, "cwfa_projection_compose_f32: null pointer");
    CWFA_REQUIRE(B >= 0 && D >= 0 && H >= 0 && W >= 0 && border >= 0 && B <= 65535, CWFA_E_SHAPE, "cwfa_projection_compose_f32: bad shape");
    CWFA_REQUIRE(depth_scale >= 1, CWFA_E_INVAL, "cwfa_projection_compose_f32: the depth scaling factor must be >= 1");
    CWFA_REQUIRE(H == W, CWFA_E_SHAPE, "cwfa_projection_compose_f32: the composite needs a square plane (H=%d, W=%d): the reference sizes "
                 "the over-H image by H and stores it W wide", H, W);
    if (B == 0 || D == 0 || H == 0) return CWFA_OK;
    const int64_t s4 = (int64_t)D * depth_scale, side = H + s4 + border;
    CWFA_REQUIRE(side * side < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_projection_compose_f32: image too large");
    const float dscale = (float)D / (float)s4;
    hipLaunchKernelGGL(compose_kernel, dim3((unsigned)((side * side + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, zproj, xproj,
                       yproj, fill, out, D, H, W, (int)s4, border, scale_bars, dscale);
    CWFA_LAUNCH_CHECK("cwfa_projection_compose_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ ROI traces
// One wave per (box, time step); the boxes of a launch travel in the kernel arguments (checked on the host, no device table).
#define ROI_CHUNK 128
struct RoiChunk {
    int box[ROI_CHUNK][6];
};

__global__ __launch_bounds__(64) void roi_means_kernel(const float* __restrict__ x, int64_t t_stride, int H, int W, RoiChunk boxes,
                                                       double* __restrict__ out, int T) {
    const int t = blockIdx.x;
    const int* bx = boxes.box[blockIdx.y];
    const int z0 = bx[0], nz = bx[1] - bx[0], y0 = bx[2], ny = bx[3] - bx[2], x0 = bx[4], nx = bx[5] - bx[4];
    const int cnt = nz * ny * nx;
    const float* p = x + t * t_stride;
    double s = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 64) {
        const int xx = i % nx, yy = (i / nx) % ny, zz = i / (nx * ny);
        s += (double)p[((int64_t)(z0 + zz) * H + y0 + yy) * W + x0 + xx];
    }
    s = cwfa_wave_sum(s);
    if (threadIdx.x == 0) out[(int64_t)blockIdx.y * T + t] = cnt ? s / (double)cnt : (double)NAN;
}

extern "C" int cwfa_roi_means_f32(const float* x, const int32_t* boxes, double* out, int T, int D, int H, int W, int N, int64_t t_stride,
                                  void* stream) {
    CWFA_REQUIRE(x && out && (boxes || N == 0), CWFA_E_INVAL, "cwfa_roi_means_f32: null pointer");
    CWFA_REQUIRE(T >= 0 && D >= 0 && H >= 0 && W >= 0 && N >= 0, CWFA_E_SHAPE, "cwfa_roi_means_f32: bad shape");
    CWFA_REQUIRE(t_stride >= 0 && (T <= 1 || t_stride >= (int64_t)D * H * W), CWFA_E_INVAL, "cwfa_roi_means_f32: time stride smaller than a volume");
    for (int i = 0; i < N; ++i) {
        const int32_t* b = boxes + 6 * i;
        CWFA_REQUIRE(0 <= b[0] && b[0] <= b[1] && b[1] <= D && 0 <= b[2] && b[2] <= b[3] && b[3] <= H && 0 <= b[4] && b[4] <= b[5] && b[5] <= W,
                     CWFA_E_INVAL, "cwfa_roi_means_f32: box %d [%d,%d) x [%d,%d) x [%d,%d) is not inside the %d x %d x %d volume", i, b[0],
                     b[1], b[2], b[3], b[4], b[5], D, H, W);
        CWFA_REQUIRE((int64_t)(b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4]) < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_roi_means_f32: box %d too large", i);
    }
    if (T == 0 || N == 0) return CWFA_OK;
    for (int n0 = 0; n0 < N; n0 += ROI_CHUNK) {
        const int m = N - n0 < ROI_CHUNK ? N - n0 : ROI_CHUNK;
        RoiChunk ck;
        for (int i = 0; i < m; ++i)
            for (int k = 0; k < 6; ++k) ck.box[i][k] = boxes[6 * (n0 + i) + k];
        for (int i = m; i < ROI_CHUNK; ++i)
            for (int k = 0; k < 6; ++k) ck.box[i][k] = 0;
        hipLaunchKernelGGL(roi_means_kernel, dim3(T, m), dim3(64), 0, (hipStream_t)stream, x, t_stride, H, W, ck, out + (int64_t)n0 * T, T);
        CWFA_LAUNCH_CHECK("cwfa_roi_means_f32");
    }
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ k-th smallest positive
// Radix selection on the bit patterns (positive fp32 values order like their bits): four passes of eight bits, most significant
// first.  A pass counts, per value of its digit, the positive elements whose higher digits equal the prefix chosen so far -- an
// LDS histogram per block (runs of equal digits are counted in registers first: real volumes share their exponent), then one
// vector atomic add per bin and block; a one-block kernel then walks the 256 counts and extends the prefix.
// NONZERO: the same selection over the elements != 0 of either sign (both zeros excluded), on the order-preserving key of the
// bit pattern: negative values with every bit flipped, the others with the sign bit set.
struct SelState {
    unsigned prefix;
    int bad;
    unsigned long long k, count;
};

__device__ __forceinline__ unsigned sel_key(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ unsigned sel_unkey(unsigned k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

template <bool NONZERO>
__global__ __launch_bounds__(256) void select_hist_kernel(const float* __restrict__ x, int64_t n, int64_t x_bs, int pass,
                                                          unsigned long long* __restrict__ hist, const SelState* __restrict__ st, int vec) {
    __shared__ unsigned long long lh[256];
    if (pass && st->bad) return;
    lh[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned prefix = pass ? st->prefix : 0;
    int cur = -1;
    unsigned long long run = 0;
    eval_stream<false>(x + blockIdx.y * x_bs, nullptr, n, vec, [&](float v, float) {
        const unsigned u = NONZERO ? sel_key(f2u(v)) : f2u(v);
        if ((NONZERO ? v != 0.f : (int)u > 0) && (pass == 0 || (u >> (shift + 8)) == prefix)) {
            const int bin = (u >> shift) & 255;
            if (bin == cur) {
                ++run;
            } else {
                if (run) atomicAdd(&lh[cur], run);
                cur = bin, run = 1;
            }
        }
    });
    if (run) atomicAdd(&lh[cur], run);
    __syncthreads();
    if (lh[threadIdx.x]) atomicAdd(&hist[pass * 256 + threadIdx.x], lh[threadIdx.x]);
}

__global__ void select_pick_kernel(const unsigned long long* __restrict__ hist, SelState* __restrict__ st, int pass, long long k_in,
                                   float* __restrict__ value, long long* __restrict__ count, int nonzero) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (pass == 0) {
        unsigned long long total = 0;
        for (int b = 0; b < 256; ++b) total += hist[b];
        st->count = total;
        *count = (long long)total;
        const unsigned long long k = k_in < 0 ? (total ? (total - 1) / 2 : 0) : (unsigned long long)k_in;
        st->k = k;
        st->prefix = 0;
        st->bad = k >= total;
        if (st->bad) *value = NAN;
    }
    if (st->bad) return;
    unsigned long long k = st->k;
    for (int b = 0; b < 256; ++b) {
        const unsigned long long c = hist[pass * 256 + b];
        if (k < c) {
            st->prefix = (st->prefix << 8) | (unsigned)b;
            st->k = k;
            break;
        }
        k -= c;
    }
    if (pass == 3) *value = u2f(nonzero ? sel_unkey(st->prefix) : st->prefix);
}

template <bool NONZERO>
static int select_run(const char* name, const float* x, int B, int64_t n, int64_t x_bs, int64_t k, float* value, int64_t* count,
                      void* workspace, void* stream) {
    CWFA_REQUIRE(x && value && count && workspace, CWFA_E_INVAL, "%s: null pointer", name);
    CWFA_REQUIRE(B >= 0 && n >= 0 && B <= 65535 && n < ((int64_t)1 << 45), CWFA_E_SHAPE, "%s: bad shape", name);
    CWFA_REQUIRE(x_bs >= 0 && (B <= 1 || x_bs >= n), CWFA_E_INVAL, "%s: batch stride smaller than a sample", name);
    CWFA_REQUIRE(k >= -1, CWFA_E_INVAL, "%s: k must be >= 0, or -1 for the lower median", name);
    CWFA_REQUIRE(k < (B * n > 0 ? B * n : 1), CWFA_E_INVAL, "%s: k = %lld is not below the element count %lld", name, (long long)k,
                 (long long)(B * n));
    if (B == 0 || n == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(workspace, 0, CWFA_SELECT_WORKSPACE_BYTES, st) != hipSuccess) {
        cwfa_set_error("%s: clearing the workspace failed", name);
        return CWFA_E_HIP;
    }
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(workspace);
    SelState* state = reinterpret_cast<SelState*>(hist + 4 * 256);
    const int splits = eval_splits(n, B);
    const int vec = eval_vec(B, x, x_bs, nullptr, 0);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(select_hist_kernel<NONZERO>, dim3(splits, B), dim3(256), 0, st, x, n, x_bs, pass, hist, state, vec);
        CWFA_LAUNCH_CHECK(name);
        hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(64), 0, st, hist, state, pass, (long long)k, value, reinterpret_cast<long long*>(count),
                           (int)NONZERO);
        CWFA_LAUNCH_CHECK(name);
    }
    return CWFA_OK;
}

extern "C" int cwfa_select_positive_f32(const float* x, int B, int64_t n, int64_t x_bs, int64_t k, float* value, int64_t* count,
                                        void* workspace, void* stream) {
    return select_run<false>("cwfa_select_positive_f32", x, B, n, x_bs, k, value, count, workspace, stream);
}

// Tmp[Tmp != 0].median() of the ratio image (utils.py:702-703), which is negative where the background-subtracted image is
extern "C" int cwfa_select_nonzero_f32(const float* x, int B, int64_t n, int64_t x_bs, int64_t k, float* value, int64_t* count,
                                       void* workspace, void* stream) {
    return select_run<true>("cwfa_select_nonzero_f32", x, B, n, x_bs, k, value, count, workspace, stream);
}
