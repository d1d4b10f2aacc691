// The data preparation pass in front of every run (reference utils.py:84-220, XLFMDataset.py:15-40,101-104,160-162,251-395):
// centre crop and thresholds of the fp16 volumes, clean-up and crop of the raw frames, torch.histogram's counts for the quantile
// clamp, the in-place clamp / standardise / normalise maps, and the moments behind the dataset statistics.  All HBM-bound
// streaming kernels.  Built with -ffp-contract=off: every fp32 operation is rounded separately, like the reference's on the CPU.
#include <math.h>
#include "common.h"

// Every element of x[0..n) once, over the whole grid.  `vec`: the base is 16-byte aligned, so the body runs on 16-byte loads,
// four in flight per thread; the ragged end on scalar loads.  Which thread sees which element is a fixed function of n and
// the launch shape (the float64 sums built on it are bitwise reproducible).
template <class F>
__device__ __forceinline__ void prep_stream(const float* __restrict__ p, int64_t n, int vec, F&& f) {
    const int64_t nt = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t done = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        const f32x4* p4 = reinterpret_cast<const f32x4*>(p);
        int64_t i = tid;
        for (; i + 3 * nt < n4; i += 4 * nt) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = p4[i + u * nt];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) f(v[u][j]);
        }
        for (; i < n4; i += nt) {
            const f32x4 v = p4[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) f(v[j]);
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += nt) f(p[i]);
}

// blocks of the streaming kernels: >= 4096 elements per block of 256 threads, the chip several times over at most
static inline int prep_blocks(int64_t n, int cap) {
    int64_t s = (n + 4095) / 4096;
    if (s > cap) s = cap;
    return s < 1 ? 1 : (int)s;
}

// ------------------------------------------------------------------------------------------------ volumes
// fp32 values order like these keys as unsigned integers (negative values included): the maximum by integer atomics, exact and
// independent of the order.  Key 0 is below the key of every value (-inf is 0x007fffff).
__device__ __forceinline__ unsigned prep_key(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float prep_unkey(unsigned k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// element index of the group g of V consecutive output columns in the source: crop of [ND, H0, W0] to [ND, H, W]
template <int V>
__device__ __forceinline__ int64_t prep_crop_src(int64_t g, int H0, int W0, int H, int W, int oh, int ow, int64_t* dst) {
    const int wg = W / V;
    const int64_t row = g / wg;
    const int col = (int)(g % wg) * V;
    const int64_t nd = row / H;
    const int h = (int)(row % H);
    *dst = row * W + col;
    return (nd * H0 + h + oh) * W0 + ow + col;
}

template <int V>
__global__ __launch_bounds__(256) void vol_max_kernel(const _Float16* __restrict__ x, int64_t groups, int H0, int W0, int H, int W, int oh,
                                                      int ow, unsigned* __restrict__ key) {
    __shared__ unsigned red[4];
    float m = -INFINITY;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        int64_t dst;
        const int64_t src = prep_crop_src<V>(g, H0, W0, H, W, oh, ow, &dst);
#pragma unroll
        for (int j = 0; j < V; ++j) m = fmaxf(m, (float)x[src + j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = prep_key(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned k = red[0];
        for (int i = 1; i < 4; ++i) k = k > red[i] ? k : red[i];
        atomicMax(key, k);
    }
}

__global__ void vol_max_finish_kernel(const unsigned* __restrict__ key, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = prep_unkey(*key);
}

// The threshold step of load_process_volume on one fp16 value, every comparison in fp32 and every stored value an fp16 one:
// TWO: v < t0 -> 0, then v >= t1 -> t1 (t1 already rounded to fp16 by the host); LE: v <= t0 -> 0 (t0 = ths * max, formed on the
// host); MAXNORM: q = fp16(v / max) (fp32 quotient, round to nearest even), then q < t0 -> 0.
__device__ __forceinline__ _Float16 prep_vol_map(_Float16 hv, int mode, float t0, float t1, float mx) {
    float v = (float)hv;
    switch (mode) {
        case CWFA_PREP_VOL_TWO:
            if (v < t0) v = 0.f;
            if (v >= t1) v = t1;
            return (_Float16)v;
        case CWFA_PREP_VOL_LE:
            return v <= t0 ? (_Float16)0.f : hv;
        case CWFA_PREP_VOL_MAXNORM: {
            const _Float16 q = (_Float16)(v / mx);
            return (float)q < t0 ? (_Float16)0.f : q;
        }
        default:
            return hv;
    }
}

template <int V, class OUT>
__global__ __launch_bounds__(256) void vol_prep_kernel(const _Float16* __restrict__ x, OUT* __restrict__ out, int64_t groups, int H0, int W0,
                                                       int H, int W, int oh, int ow, int mode, float t0, float t1,
                                                       const float* __restrict__ maxbuf) {
    const float mx = mode == CWFA_PREP_VOL_MAXNORM ? *maxbuf : 1.f;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        int64_t dst;
        const int64_t src = prep_crop_src<V>(g, H0, W0, H, W, oh, ow, &dst);
        OUT r[V];
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = (OUT)prep_vol_map(x[src + j], mode, t0, t1, mx);
        if constexpr (V == 4) {
            typedef OUT out4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<out4*>(out + dst) = out4{r[0], r[1], r[2], r[3]};
        } else {
            out[dst] = r[0];
        }
    }
}

extern "C" int cwfa_prep_volumes_f16(const void* x, void* out, float* maxbuf, int N, int D, int H0, int W0, int H, int W, int off_h,
                                     int off_w, int mode, float t0, float t1, int out_f16, void* stream) {
    CWFA_REQUIRE(mode >= CWFA_PREP_VOL_NONE && mode <= CWFA_PREP_VOL_MAX_ONLY, CWFA_E_INVAL, "cwfa_prep_volumes_f16: unknown mode %d", mode);
    const bool need_max = mode == CWFA_PREP_VOL_MAXNORM || mode == CWFA_PREP_VOL_MAX_ONLY;
    CWFA_REQUIRE(x && (out || mode == CWFA_PREP_VOL_MAX_ONLY) && (maxbuf || !need_max), CWFA_E_INVAL, "cwfa_prep_volumes_f16: null pointer");
    CWFA_REQUIRE(N >= 0 && D >= 0 && H0 >= 0 && W0 >= 0 && H >= 0 && W >= 0, CWFA_E_SHAPE, "cwfa_prep_volumes_f16: negative size");
    CWFA_REQUIRE(off_h >= 0 && off_w >= 0 && (int64_t)off_h + H <= H0 && (int64_t)off_w + W <= W0, CWFA_E_SHAPE,
                 "cwfa_prep_volumes_f16: the crop [%d:%d, %d:%d] is not inside the %d x %d plane", off_h, off_h + H, off_w, off_w + W, H0, W0);
    const int64_t n = (int64_t)N * D * H * W;
    if (n == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    const _Float16* xp = reinterpret_cast<const _Float16*>(x);
    // four columns per thread where the rows allow it and the stores are aligned
    const int v4 = (W & 3) == 0 && (mode == CWFA_PREP_VOL_MAX_ONLY || cwfa_aligned16(out));
    const int64_t groups = v4 ? n >> 2 : n;
    const int blocks = prep_blocks(groups * 4, 8192);
    if (need_max) {
        unsigned* key = reinterpret_cast<unsigned*>(maxbuf);
        if (hipMemsetAsync(key, 0, sizeof(unsigned), st) != hipSuccess) {
            cwfa_set_error("cwfa_prep_volumes_f16: clearing the maximum failed");
            return CWFA_E_HIP;
        }
        if (v4)
            hipLaunchKernelGGL(vol_max_kernel<4>, dim3(blocks), dim3(256), 0, st, xp, groups, H0, W0, H, W, off_h, off_w, key);
        else
            hipLaunchKernelGGL(vol_max_kernel<1>, dim3(blocks), dim3(256), 0, st, xp, groups, H0, W0, H, W, off_h, off_w, key);
        CWFA_LAUNCH_CHECK("cwfa_prep_volumes_f16");
        hipLaunchKernelGGL(vol_max_finish_kernel, dim3(1), dim3(64), 0, st, key, maxbuf + 1);
        CWFA_LAUNCH_CHECK("cwfa_prep_volumes_f16");
        if (mode == CWFA_PREP_VOL_MAX_ONLY) return CWFA_OK;
    }
    const float* mb = need_max ? maxbuf + 1 : nullptr;
#define PREP_VOL_LAUNCH(V, OUT)                                                                                                          \
    hipLaunchKernelGGL((vol_prep_kernel<V, OUT>), dim3(blocks), dim3(256), 0, st, xp, reinterpret_cast<OUT*>(out), groups, H0, W0, H, W, \
                       off_h, off_w, mode, t0, t1, mb)
    if (out_f16) {
        if (v4) PREP_VOL_LAUNCH(4, _Float16);
        else PREP_VOL_LAUNCH(1, _Float16);
    } else {
        if (v4) PREP_VOL_LAUNCH(4, float);
        else PREP_VOL_LAUNCH(1, float);
    }
#undef PREP_VOL_LAUNCH
    CWFA_LAUNCH_CHECK("cwfa_prep_volumes_f16");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ frames
// XLFMDataset.py:101-104,160-162 per element: NaN -> 0, clip to [0, 50000] (so +inf -> 50000, -inf -> 0), a round trip through
// fp16 (round to nearest even), and the index map of pad_img_to_min + center_crop as one offset pair; positions outside the
// source are 0.
__global__ __launch_bounds__(256) void frames_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t total, int h, int w, int S0,
                                                     int S1, int oy, int ox) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % S1);
        const int64_t t = i / S1;
        const int r = (int)(t % S0);
        const int64_t n = t / S0;
        const int sr = r + oy, sc = c + ox;
        float v = 0.f;
        if (sr >= 0 && sr < h && sc >= 0 && sc < w) {
            v = x[(n * h + sr) * w + sc];
            v = v != v ? 0.f : v;
            v = v < 0.f ? 0.f : v;
            v = v > 50000.f ? 50000.f : v;
            v = (float)(_Float16)v;
        }
        out[i] = v;
    }
}

extern "C" int cwfa_prep_frames_f32(const float* x, float* out, int N, int h, int w, int S0, int S1, int off_y, int off_x, void* stream) {
    CWFA_REQUIRE(x && out, CWFA_E_INVAL, "cwfa_prep_frames_f32: null pointer");
    CWFA_REQUIRE(N >= 0 && h >= 0 && w >= 0 && S0 >= 0 && S1 >= 0, CWFA_E_SHAPE, "cwfa_prep_frames_f32: negative size");
    CWFA_REQUIRE(off_y > -(1 << 30) && off_y < (1 << 30) && off_x > -(1 << 30) && off_x < (1 << 30), CWFA_E_INVAL,
                 "cwfa_prep_frames_f32: offset out of range");
    const int64_t total = (int64_t)N * S0 * S1;
    if (total == 0) return CWFA_OK;
    hipLaunchKernelGGL(frames_kernel, dim3(prep_blocks(total * 4, 8192)), dim3(256), 0, (hipStream_t)stream, x, out, total, h, w, S0, S1, off_y,
                       off_x);
    CWFA_LAUNCH_CHECK("cwfa_prep_frames_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ histogram
// torch.histogram's bin of x on the CPU (ATen HistogramKernel, linear bins with local search): the position by fp32 arithmetic,
// then the exact answer among the neighbouring edges -- the last edge <= x within edges[pos-1 .. pos+1] -- because the rounded
// position is off by one for values near an edge (and for every value ON an edge that the arithmetic puts just below it).  The
// top edge belongs to the last bin.  x lies in [lo, hi].
__device__ __forceinline__ int prep_bin(float x, float lo, float range, float fbins, int bins, const float* edges) {
    int pos = (int)((x - lo) / range * fbins);
    pos = pos < 0 ? 0 : (pos > bins ? bins : pos);
    const int a = pos > 0 ? pos - 1 : 0, b = pos + 2 < bins + 1 ? pos + 2 : bins + 1;
    int cnt = 0;
    for (int k = a; k < b; ++k) cnt += edges[k] <= x ? 1 : 0;
    int bin = a + cnt - 1;
    bin = bin > bins - 1 ? bins - 1 : bin;
    return bin < 0 ? 0 : bin;
}

#define HIST_THREADS 512
#define HIST_BLOCKS 512

// A persistent grid; every block counts its share into a private LDS table next to an LDS copy of the edges and adds its
// occupied bins to the int64 table at the end: blocks x occupied bins global atomics, not n.  Volumes are mostly background:
// the elements equal to lo (bin 0) are counted in a register and never reach the LDS.  Integer atomics only: the counts are
// exact and independent of the order.
__global__ __launch_bounds__(HIST_THREADS) void hist_kernel(const float* __restrict__ x, int64_t n, float lo, float hi, int bins,
                                                            const float* __restrict__ edges, unsigned long long* __restrict__ counts, int vec) {
    __shared__ unsigned lh[CWFA_PREP_MAX_BINS];
    __shared__ float le[CWFA_PREP_MAX_BINS + 1];
    for (int i = threadIdx.x; i < bins; i += HIST_THREADS) lh[i] = 0;
    for (int i = threadIdx.x; i <= bins; i += HIST_THREADS) le[i] = edges[i];
    __syncthreads();
    const float range = hi - lo, fbins = (float)bins;
    unsigned nlo = 0;
    prep_stream(x, n, vec, [&](float v) {
        if (!(v >= lo && v <= hi)) return;                  // outside the range (or NaN): not counted, as torch skips them
        if (v == lo) {
            ++nlo;
            return;
        }
        atomicAdd(&lh[prep_bin(v, lo, range, fbins, bins, le)], 1u);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nlo += __shfl_xor(nlo, o, 64);
    if ((threadIdx.x & 63) == 0 && nlo) atomicAdd(&lh[0], nlo);
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += HIST_THREADS)
        if (lh[i]) atomicAdd(&counts[i], (unsigned long long)lh[i]);
}

extern "C" int cwfa_histogram_f32(const float* x, int64_t n, float lo, float hi, const float* edges, int bins, int64_t* counts,
                                  int accumulate, void* stream) {
    CWFA_REQUIRE(counts && edges && (x || n == 0), CWFA_E_INVAL, "cwfa_histogram_f32: null pointer");
    CWFA_REQUIRE(n >= 0 && n < ((int64_t)1 << 40), CWFA_E_SHAPE, "cwfa_histogram_f32: bad element count");
    CWFA_REQUIRE(bins >= 1 && bins <= CWFA_PREP_MAX_BINS, CWFA_E_INVAL, "cwfa_histogram_f32: bins = %d is not in 1 .. %d", bins,
                 CWFA_PREP_MAX_BINS);
    CWFA_REQUIRE(isfinite(lo) && isfinite(hi) && lo < hi, CWFA_E_INVAL, "cwfa_histogram_f32: the range [%g, %g] must be finite and not empty",
                 (double)lo, (double)hi);
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate && hipMemsetAsync(counts, 0, sizeof(int64_t) * bins, st) != hipSuccess) {
        cwfa_set_error("cwfa_histogram_f32: clearing the counts failed");
        return CWFA_E_HIP;
    }
    if (n == 0) return CWFA_OK;
    // a block's share stays far below 2^32 (n < 2^40 over up to 512 blocks of >= 8192 elements)
    int64_t blocks = (n + 8191) / 8192;
    blocks = blocks > HIST_BLOCKS ? HIST_BLOCKS : blocks;
    CWFA_REQUIRE(n / blocks < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_histogram_f32: too many elements for the 32-bit block counters");
    hipLaunchKernelGGL(hist_kernel, dim3((unsigned)blocks), dim3(HIST_THREADS), 0, st, x, n, lo, hi, bins, edges,
                       reinterpret_cast<unsigned long long*>(counts), (int)cwfa_aligned16(x));
    CWFA_LAUNCH_CHECK("cwfa_histogram_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ in-place maps
// CLAMP_ZERO: x > a -> a (flag bit 0), then x < b -> 0 (flag bit 1): the quantile clamp and the image threshold of load_XLFM_data;
// SUB_DIV: (x - a) / b, `standarize`; DIV_MUL: x / a * b, `normalize_datasets`.  IEEE fp32 operations in the reference's order.
__device__ __forceinline__ float prep_map(float v, int mode, float a, float b, int flags) {
    switch (mode) {
        case CWFA_PREP_SUB_DIV: return (v - a) / b;
        case CWFA_PREP_DIV_MUL: return v / a * b;
        default:
            if ((flags & 1) && v > a) v = a;
            if ((flags & 2) && v < b) v = 0.f;
            return v;
    }
}

__global__ __launch_bounds__(256) void apply_kernel(float* __restrict__ x, int64_t n, int mode, float a, float b, int flags, int vec) {
    const int64_t nt = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t done = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        f32x4* x4 = reinterpret_cast<f32x4*>(x);
        for (int64_t i = tid; i < n4; i += nt) {
            f32x4 v = x4[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = prep_map(v[j], mode, a, b, flags);
            x4[i] = v;
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += nt) x[i] = prep_map(x[i], mode, a, b, flags);
}

extern "C" int cwfa_prep_apply_f32(float* x, int64_t n, int mode, float a, float b, int flags, void* stream) {
    CWFA_REQUIRE(x || n == 0, CWFA_E_INVAL, "cwfa_prep_apply_f32: null pointer");
    CWFA_REQUIRE(n >= 0, CWFA_E_SHAPE, "cwfa_prep_apply_f32: negative size");
    CWFA_REQUIRE(mode >= CWFA_PREP_CLAMP_ZERO && mode <= CWFA_PREP_DIV_MUL, CWFA_E_INVAL, "cwfa_prep_apply_f32: unknown mode %d", mode);
    CWFA_REQUIRE(mode != CWFA_PREP_CLAMP_ZERO || (flags >= 0 && flags <= 3), CWFA_E_INVAL, "cwfa_prep_apply_f32: flags is a mask of bits 0..1");
    if (n == 0) return CWFA_OK;
    hipLaunchKernelGGL(apply_kernel, dim3(prep_blocks(n, 8192)), dim3(256), 0, (hipStream_t)stream, x, n, mode, a, b, flags,
                       (int)cwfa_aligned16(x));
    CWFA_LAUNCH_CHECK("cwfa_prep_apply_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ moments
// sum (x - c) and sum (x - c)^2 in float64 (the difference of an fp32 value and c is rounded once, the square once).  Per block
// the two sums go to a slab; the finish kernel adds the slab in a fixed order: bitwise reproducible, no float atomics.
#define MOM_MAX_BLOCKS (CWFA_PREP_MOMENTS_WORKSPACE / 2)

__global__ __launch_bounds__(256) void moments_kernel(const float* __restrict__ x, int64_t n, double c, double* __restrict__ slab, int vec) {
    __shared__ double red[16];
    double s1 = 0.0, s2 = 0.0;
    prep_stream(x, n, vec, [&](float v) {
        const double d = (double)v - c;
        s1 += d;
        s2 += d * d;
    });
    s1 = cwfa_block_sum(s1, red);
    s2 = cwfa_block_sum(s2, red);
    if (threadIdx.x == 0) slab[2 * blockIdx.x] = s1, slab[2 * blockIdx.x + 1] = s2;
}

__global__ __launch_bounds__(256) void moments_finish_kernel(const double* __restrict__ slab, int blocks, double count, int accumulate,
                                                             double* __restrict__ out) {
    __shared__ double red[16];
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < blocks; i += blockDim.x) s1 += slab[2 * i], s2 += slab[2 * i + 1];
    s1 = cwfa_block_sum(s1, red);
    s2 = cwfa_block_sum(s2, red);
    if (threadIdx.x == 0) {
        out[0] = (accumulate ? out[0] : 0.0) + s1;
        out[1] = (accumulate ? out[1] : 0.0) + s2;
        out[2] = (accumulate ? out[2] : 0.0) + count;
    }
}

extern "C" int cwfa_moments_f64(const float* x, int64_t n, double c, double* out, double* workspace, int accumulate, void* stream) {
    CWFA_REQUIRE(out && workspace && (x || n == 0), CWFA_E_INVAL, "cwfa_moments_f64: null pointer");
    CWFA_REQUIRE(n >= 0 && n < ((int64_t)1 << 52), CWFA_E_SHAPE, "cwfa_moments_f64: bad element count");
    CWFA_REQUIRE(isfinite(c), CWFA_E_INVAL, "cwfa_moments_f64: the shift must be finite");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = n ? prep_blocks(n, MOM_MAX_BLOCKS) : 0;
    if (n) {
        hipLaunchKernelGGL(moments_kernel, dim3(blocks), dim3(256), 0, st, x, n, c, workspace, (int)cwfa_aligned16(x));
        CWFA_LAUNCH_CHECK("cwfa_moments_f64");
    }
    hipLaunchKernelGGL(moments_finish_kernel, dim3(1), dim3(256), 0, st, workspace, blocks, (double)n, accumulate, out);
    CWFA_LAUNCH_CHECK("cwfa_moments_f64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ per-voxel mean / std
// Over the N samples of [N, m]: float64 sums of the differences to the first sample (exact differences of fp32 values), so a
// voxel with a large mean and a small spread keeps its variance.  mean = x0 + S1 / N, var = (S2 - S1^2 / N) / (N - 1): N = 1
// gives 0 / 0 = NaN, as torch's unbiased std does.
template <int V>
__global__ __launch_bounds__(256) void stack_kernel(const float* __restrict__ x, float* __restrict__ mean, float* __restrict__ sd, int N,
                                                    int64_t groups, int64_t ss) {
    typedef float vec __attribute__((ext_vector_type(V)));
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const float* p = x + g * V;
        const vec x0 = *reinterpret_cast<const vec*>(p);
        double s1[V], s2[V];
#pragma unroll
        for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.0;
        for (int s = 1; s < N; ++s) {
            const vec v = *reinterpret_cast<const vec*>(p + s * ss);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double d = (double)v[j] - (double)x0[j];
                s1[j] += d;
                s2[j] += d * d;
            }
        }
        vec mo, so;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            mo[j] = (float)((double)x0[j] + s1[j] / (double)N);
            const double var = (s2[j] - s1[j] * s1[j] / (double)N) / (double)(N - 1);
            so[j] = (float)sqrt(var < 0.0 ? 0.0 : var);
        }
        *reinterpret_cast<vec*>(mean + g * V) = mo;
        *reinterpret_cast<vec*>(sd + g * V) = so;
    }
}

extern "C" int cwfa_stack_mean_std_f32(const float* x, float* mean, float* std, int N, int64_t m, int64_t x_ss, void* stream) {
    CWFA_REQUIRE(x && mean && std, CWFA_E_INVAL, "cwfa_stack_mean_std_f32: null pointer");
    CWFA_REQUIRE(N >= 1 && m >= 0, CWFA_E_SHAPE, "cwfa_stack_mean_std_f32: needs at least one sample and a non-negative size");
    CWFA_REQUIRE(N == 1 || x_ss >= m, CWFA_E_INVAL, "cwfa_stack_mean_std_f32: sample stride smaller than a sample");
    if (m == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    if ((m & 3) == 0 && (N == 1 || (x_ss & 3) == 0) && cwfa_aligned16(x) && cwfa_aligned16(mean) && cwfa_aligned16(std))
        hipLaunchKernelGGL(stack_kernel<4>, dim3(prep_blocks(m * 4, 8192)), dim3(256), 0, st, x, mean, std, N, m >> 2, x_ss);
    else
        hipLaunchKernelGGL(stack_kernel<1>, dim3(prep_blocks(m * 16, 8192)), dim3(256), 0, st, x, mean, std, N, m, x_ss);
    CWFA_LAUNCH_CHECK("cwfa_stack_mean_std_f32");
    return CWFA_OK;
}
