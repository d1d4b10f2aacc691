// What a user reads from the traces behind extract_traces, on float64 [N, T] rows with a row stride in elements:
// a sliding-window quantile (the running-percentile baseline of dF/F), per-row order statistics (the two medians of the noise level) and
// the exact non-negative AR(1) deconvolution by the pool algorithm (Friedrich, Zhou & Paninski 2017).  Built with -ffp-contract=off:
// every float64 operation is rounded separately, in the order of the numpy restatement.
#include <math.h>
#include "common.h"

// ------------------------------------------------------------------------------------------------ order-preserving keys
// The order of sparse_ops.hip, widened to 64 bits: the unsigned image of the float64 bits of v + 0.0, formed on the bits, all 64 of
// them.  Every NaN of either sign takes the all-ones key, which no other value has (it would be the image of the bits 0x7fff.., a
// NaN), sorts last and comes back as the canonical quiet NaN.
__device__ __forceinline__ uint64_t tr_key(double v) {
    uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint64_t mag = u & 0x7fffffffffffffffull;
    u = mag == 0 ? 0ull : u;
    const uint64_t k = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return mag > 0x7ff0000000000000ull ? ~0ull : k;
}
__device__ __forceinline__ double tr_unkey(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __builtin_bit_cast(double, k == ~0ull ? 0x7ff8000000000000ull : u);
}

// ------------------------------------------------------------------------------------------------ sliding quantile, the LDS form
// A workgroup owns a row and a segment of SQ_TILE outputs, a lane an output.  It stages the keys of the segment and its halo -- the M
// <= SQ_TILE + 2h samples any of its windows touches -- and replaces each by its rank in the staged set, rank = the number of staged
// keys below it: equal keys share a rank, a rank is below M, and the order of the ranks is the order of the keys.  The window's k-th
// smallest rank is then found from the top bit of ceil(log2 M) down, counting 16-bit entries.  byrank[r] holds one staged index of
// rank r (the writers of one slot hold equal keys: whichever wins, the value read back is the same), which maps the result to the
// element of the series.
//   Counting.  The ranks lie at place r = sample - (t0 - h); places outside the row hold 0xffff, which is below no candidate, so
//   every window of the segment is the 2h + 1 places from its lane's number on.  An LDS read that is not aligned to its size is an
//   order of magnitude slower on gfx950 (section 5.1), so a lane does not read its window from its own place: the eight lanes l,
//   l + 1, .. l + 7 (l a multiple of 8) read the same SQ_GROUPS(h) aligned 16-byte groups from place l on -- a wave reads 8 distinct
//   groups per ds_read_b128, the rest is broadcast -- and a lane takes off what it counted before its window (up to 7 places) and
//   behind it (up to 14) with single 2-byte reads.
//   Ranking: a thread keeps SQ_RPT of its keys in registers and passes once over the staged keys, every lane reading the same address.
//   LDS: 8 + 2 bytes per staged sample (key, byrank; M rounded up to 8) and 2 per place of the SQ_TILE + 8 SQ_GROUPS(h) ranks:
//   64 528 bytes at h = SQ_MAX_HALF, below the 64 KiB a kernel gets without asking.
//   LDS reads per output and key bit: SQ_GROUPS(h) of 16 bytes and 21 of 2 bytes; for the ranking M * ceil(M / (SQ_TILE * SQ_RPT))
//   of 8 bytes, every lane of a wave at the same address.
#define SQ_TILE 256
#define SQ_RPT 4
#define SQ_MAX_HALF 2560
#define SQ_GROUPS(h) ((2 * (h) + 1 + 7 + 7) / 8)
#define SQ_PLACES(h) (SQ_TILE + 8 * SQ_GROUPS(h))
static_assert(((SQ_TILE + 2 * SQ_MAX_HALF + 7) & ~7) * 10 + SQ_PLACES(SQ_MAX_HALF) * 2 <= 65536, "the LDS form's stage exceeds 64 KiB");

__global__ __launch_bounds__(SQ_TILE) void sq_lds_kernel(const double* __restrict__ x, int T, int64_t stride, int h, int p, int segs,
                                                         int mpad, double* __restrict__ out) {
    extern __shared__ uint64_t sq_lds[];
    uint64_t* keys = sq_lds;                                                    // [mpad]
    unsigned short* byrank = reinterpret_cast<unsigned short*>(sq_lds + mpad);  // [mpad]
    unsigned short* ranks = byrank + mpad;                                      // [SQ_PLACES(h)], place r: sample t0 - h + r; 16-byte aligned
    const int64_t n = blockIdx.x / segs;
    const int t0 = (int)(blockIdx.x % segs) * SQ_TILE;
    const int tid = threadIdx.x;
    const double* row = x + n * stride;
    const int s0 = t0 - h > 0 ? t0 - h : 0;                                     // h <= T - 1: no overflow
    const int e1 = t0 + (SQ_TILE - 1) + h < T - 1 ? t0 + (SQ_TILE - 1) + h : T - 1;
    const int M = e1 - s0 + 1;
    const int off = s0 - (t0 - h);                                              // the first staged sample's place among the ranks
    for (int i = tid; i < M; i += SQ_TILE) keys[i] = tr_key(row[s0 + i]);
    for (int r = tid; r < SQ_PLACES(h); r += SQ_TILE) ranks[r] = 0xffffu;
    __syncthreads();
    for (int base = 0; base < M; base += SQ_TILE * SQ_RPT) {
        uint64_t ki[SQ_RPT];
        int c[SQ_RPT];
#pragma unroll
        for (int q = 0; q < SQ_RPT; ++q) {
            const int i = base + q * SQ_TILE + tid;
            ki[q] = i < M ? keys[i] : 0ull;
            c[q] = 0;
        }
#pragma unroll 4
        for (int j = 0; j < M; ++j) {
            const uint64_t kj = keys[j];
#pragma unroll
            for (int q = 0; q < SQ_RPT; ++q) c[q] += kj < ki[q] ? 1 : 0;
        }
#pragma unroll
        for (int q = 0; q < SQ_RPT; ++q) {
            const int i = base + q * SQ_TILE + tid;
            if (i < M) {
                ranks[off + i] = (unsigned short)c[q];
                byrank[c[q]] = (unsigned short)i;
            }
        }
    }
    __syncthreads();
    const int t = t0 + tid;
    if (t >= T) return;                                                          // no barrier below
    const int lo = t - h > 0 ? t - h : 0, hi = t + h < T - 1 ? t + h : T - 1;
    const int k = (int)(((int64_t)p * (hi - lo)) / 100);
    const int W = 2 * h + 1, G = SQ_GROUPS(h);
    const int head = tid & 7, tail = 8 * G - head - W;                           // places counted before and behind the window
    const u32x4* grp = reinterpret_cast<const u32x4*>(ranks + (tid - head));
    const unsigned short* before = ranks + (tid - head);
    const unsigned short* behind = ranks + tid + W;
    int bits = 0;
    while ((1 << bits) < M) ++bits;
    unsigned prefix = 0;
    for (int bit = bits - 1; bit >= 0; --bit) {
        const unsigned cand = prefix | (1u << bit);
        int c = 0;
#pragma unroll 2
        for (int g = 0; g < G; ++g) {
            const u32x4 v = grp[g];
#pragma unroll
            for (int i = 0; i < 4; ++i) c += ((v[i] & 0xffffu) < cand ? 1 : 0) + ((v[i] >> 16) < cand ? 1 : 0);
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) c -= i < head && (unsigned)before[i] < cand ? 1 : 0;      // places read: inside the lane's groups
#pragma unroll
        for (int i = 0; i < 14; ++i) c -= i < tail && (unsigned)behind[i < tail ? i : 0] < cand ? 1 : 0;
        prefix = c <= k ? cand : prefix;
    }
    out[n * T + t] = tr_unkey(keys[byrank[prefix]]);
}

// ------------------------------------------------------------------------------------------------ sliding quantile, the streaming form
// Any h: a thread owns an output and counts its window straight from memory, one sweep per key bit (64 W reads per output, adjacent
// lanes on adjacent samples).  The same keys and the same rule: the cross-check of the form above and the path beyond its LDS.
__global__ __launch_bounds__(256) void sq_stream_kernel(const double* __restrict__ x, int64_t N, int T, int64_t stride, int h, int p,
                                                        double* __restrict__ out) {
    const int64_t total = N * T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t n = i / T;
        const int t = (int)(i - n * T);
        const double* row = x + n * stride;
        const int lo = t - h > 0 ? t - h : 0, hi = t + h < T - 1 ? t + h : T - 1;
        const int k = (int)(((int64_t)p * (hi - lo)) / 100);
        uint64_t prefix = 0;
        for (int bit = 63; bit >= 0; --bit) {
            const uint64_t cand = prefix | (1ull << bit);
            int c = 0;
#pragma unroll 4
            for (int j = lo; j <= hi; ++j) c += tr_key(row[j]) < cand ? 1 : 0;
            prefix = c <= k ? cand : prefix;
        }
        out[i] = tr_unkey(prefix);
    }
}

extern "C" int cwfa_sliding_quantile_limits(int* tile, int* max_half_lds) {
    CWFA_REQUIRE(tile && max_half_lds, CWFA_E_INVAL, "cwfa_sliding_quantile_limits: null pointer");
    *tile = SQ_TILE;
    *max_half_lds = SQ_MAX_HALF;
    return CWFA_OK;
}

extern "C" int cwfa_sliding_quantile_f64(const double* x, int N, int T, int64_t stride, int h, int p, double* out, int form,
                                         void* stream) {
    CWFA_REQUIRE(N >= 0 && T >= 1, CWFA_E_SHAPE, "cwfa_sliding_quantile_f64: N = %d, T = %d: N >= 0 and T >= 1 are expected", N, T);
    // the kernels form t + h and t0 + SQ_TILE - 1 + h with h <= T - 1 as ints
    CWFA_REQUIRE(T <= (1 << 30) - SQ_TILE, CWFA_E_SHAPE, "cwfa_sliding_quantile_f64: rows of more than 2^30 - %d samples", SQ_TILE);
    CWFA_REQUIRE((x && out) || N == 0, CWFA_E_INVAL, "cwfa_sliding_quantile_f64: null pointer");
    CWFA_REQUIRE(stride >= T, CWFA_E_INVAL, "cwfa_sliding_quantile_f64: row stride smaller than a row");
    CWFA_REQUIRE(h >= 0, CWFA_E_INVAL, "cwfa_sliding_quantile_f64: half window %d is negative", h);
    CWFA_REQUIRE(p >= 0 && p <= 100, CWFA_E_INVAL, "cwfa_sliding_quantile_f64: percentile %d is not in 0 .. 100", p);
    CWFA_REQUIRE(form >= 0 && form <= 2, CWFA_E_INVAL, "cwfa_sliding_quantile_f64: unknown form %d", form);
    CWFA_REQUIRE(form != 1 || h <= SQ_MAX_HALF, CWFA_E_SHAPE, "cwfa_sliding_quantile_f64: the LDS form takes a half window of at most %d, got %d",
                 SQ_MAX_HALF, h);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_sliding_quantile_f64: x and out must be 8-byte aligned");
    if (N == 0) return CWFA_OK;
    const int he = h < T - 1 ? h : T - 1;                                        // the same windows
    const int64_t segs = ((int64_t)T + SQ_TILE - 1) / SQ_TILE;
    CWFA_REQUIRE(segs * N < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_sliding_quantile_f64: more than 2^31 segments");
    hipStream_t st = (hipStream_t)stream;
    if (form == 1 || (form == 0 && he <= SQ_MAX_HALF)) {
        int64_t m = (int64_t)SQ_TILE + 2 * (int64_t)he;
        m = m < T ? m : T;
        const int mpad = (int)((m + 7) & ~(int64_t)7);                           // the ranks behind keys and byrank are 16-byte aligned
        const size_t lds = (size_t)mpad * 10 + (size_t)SQ_PLACES(he) * 2;
        hipLaunchKernelGGL(sq_lds_kernel, dim3((unsigned)(segs * N)), dim3(SQ_TILE), lds, st, x, T, stride, he, p, (int)segs, mpad, out);
    } else {
        int64_t blocks = ((int64_t)N * T + 255) / 256;
        blocks = blocks > (1 << 22) ? (1 << 22) : blocks;
        hipLaunchKernelGGL(sq_stream_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, (int64_t)N, T, stride, he, p, out);
    }
    CWFA_LAUNCH_CHECK("cwfa_sliding_quantile_f64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ row select
// The row-major float64 twin of cwfa_temporal_select: one workgroup per row, the K ranks found together from the top key bit down.
// Per bit every thread counts its samples (t = thread, thread + 256, ..) below the K candidates, a wave adds its lanes' counts, the
// four waves' counts meet in a double-buffered LDS table (one barrier per bit), and every thread adds them up for itself.
#define TRS_THREADS 256
#define TRS_WAVES (TRS_THREADS / 64)

struct trs_ranks {
    int r[4];
};

__device__ __forceinline__ int tr_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int K>
__global__ __launch_bounds__(TRS_THREADS) void trs_kernel(const double* __restrict__ x, int N, int T, int64_t stride, trs_ranks rk,
                                                          double* __restrict__ out) {
    __shared__ int part[2][TRS_WAVES][K];
    const int64_t n = blockIdx.x;
    const double* row = x + n * stride;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t prefix[K];
#pragma unroll
    for (int k = 0; k < K; ++k) prefix[k] = 0;
    for (int bit = 63; bit >= 0; --bit) {
        uint64_t cand[K];
        int c[K];
#pragma unroll
        for (int k = 0; k < K; ++k) cand[k] = prefix[k] | (1ull << bit), c[k] = 0;
#pragma unroll 4
        for (int t = threadIdx.x; t < T; t += TRS_THREADS) {
            const uint64_t key = tr_key(row[t]);
#pragma unroll
            for (int k = 0; k < K; ++k) c[k] += key < cand[k] ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = tr_wave_sum(c[k]);
            if (lane == 0) part[bit & 1][w][k] = s;
        }
        __syncthreads();
        // the table of bit is written again at bit - 2, behind the barrier of bit - 1, which every wave reaches after these reads
#pragma unroll
        for (int k = 0; k < K; ++k) {
            int tot = 0;
#pragma unroll
            for (int ww = 0; ww < TRS_WAVES; ++ww) tot += part[bit & 1][ww][k];
            prefix[k] = tot <= rk.r[k] ? cand[k] : prefix[k];
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) out[(int64_t)k * N + n] = tr_unkey(prefix[k]);
    }
}

extern "C" int cwfa_trace_select_f64(const double* x, int N, int T, int64_t stride, const int* ranks, int K, double* out, void* stream) {
    CWFA_REQUIRE(N >= 0 && T >= 1, CWFA_E_SHAPE, "cwfa_trace_select_f64: N = %d, T = %d: N >= 0 and T >= 1 are expected", N, T);
    CWFA_REQUIRE(ranks && ((x && out) || N == 0), CWFA_E_INVAL, "cwfa_trace_select_f64: null pointer");
    CWFA_REQUIRE(stride >= T, CWFA_E_INVAL, "cwfa_trace_select_f64: row stride smaller than a row");
    CWFA_REQUIRE(K >= 1 && K <= 4, CWFA_E_INVAL, "cwfa_trace_select_f64: K = %d is not in 1 .. 4", K);
    trs_ranks rk = {{0, 0, 0, 0}};
    for (int k = 0; k < K; ++k) {
        CWFA_REQUIRE(ranks[k] >= 0 && ranks[k] < T, CWFA_E_INVAL, "cwfa_trace_select_f64: rank %d is not in 0 .. %d", ranks[k], T - 1);
        rk.r[k] = ranks[k];
    }
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_trace_select_f64: x and out must be 8-byte aligned");
    if (N == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)N), block(TRS_THREADS);
    switch (K) {
        case 1: hipLaunchKernelGGL(trs_kernel<1>, grid, block, 0, st, x, N, T, stride, rk, out); break;
        case 2: hipLaunchKernelGGL(trs_kernel<2>, grid, block, 0, st, x, N, T, stride, rk, out); break;
        case 3: hipLaunchKernelGGL(trs_kernel<3>, grid, block, 0, st, x, N, T, stride, rk, out); break;
        default: hipLaunchKernelGGL(trs_kernel<4>, grid, block, 0, st, x, N, T, stride, rk, out); break;
    }
    CWFA_LAUNCH_CHECK("cwfa_trace_select_f64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ AR(1) deconvolution
// A thread owns a row: the recurrence is serial within one.  The pool stacks live in the workspace, transposed -- pool d of row n at
// [d][N] + n of V, W (float64) and L (int32) -- so that the lanes of a wave whose stacks stand at the same depth touch consecutive
// addresses.  The newest pool stays in registers: per sample the previous one is pushed, and the loop pops one pool per merge.  The
// pool starts S are not kept: the expansion walks the pools from the first and adds the lengths up.  c and s are written by the
// expansion only and read by nothing, so no pool is overwritten before it is read.
__global__ __launch_bounds__(64) void ar1_kernel(const double* __restrict__ y, int N, int T, int64_t stride, double gamma,
                                                 const double* __restrict__ lam, const double* __restrict__ pw, double* __restrict__ c,
                                                 double* __restrict__ s, int* __restrict__ pools, double* __restrict__ Vs,
                                                 double* __restrict__ Ws, int* __restrict__ Ls) {
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const double* yr = y + n * stride;
    double* cr = c + n * T;
    double* sr = s + n * T;
    const double l = lam[n];
    bool bad = !(l >= 0.0 && l < INFINITY);
    for (int t = 0; t < T; ++t) bad |= !(fabs(yr[t]) < INFINITY);
    if (bad) {
        const double nan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
        for (int t = 0; t < T; ++t) cr[t] = nan, sr[t] = nan;
        pools[n] = 0;
        return;
    }
    const double m = l * (1.0 - gamma);
    int depth = 0;                                                               // pools in memory; the newest is (v, w, len)
    double v = 0.0, w = 0.0;
    int len = 0;
    for (int t = 0; t < T; ++t) {
        if (t > 0) {
            const int64_t o = (int64_t)depth * N + n;
            Vs[o] = v, Ws[o] = w, Ls[o] = len;
            ++depth;
        }
        v = t < T - 1 ? yr[t] - m : yr[t] - l;
        w = 1.0;
        len = 1;
        while (depth > 0) {
            const int64_t o = (int64_t)(depth - 1) * N + n;
            const double pv = Vs[o];
            const int pl = Ls[o];
            const double a = pw[pl];
            if (!(v < a * pv)) break;
            const double pwt = Ws[o];
            const double wn = pwt + (a * a) * w;
            v = (pwt * pv + (a * w) * v) / wn;
            w = wn;
            len += pl;
            --depth;
        }
    }
    {
        const int64_t o = (int64_t)depth * N + n;
        Vs[o] = v, Ls[o] = len;
        ++depth;
    }
    int start = 0, plen = 0;
    double pvp = 0.0;
    for (int i = 0; i < depth; ++i) {
        const int64_t o = (int64_t)i * N + n;
        const double vi = Vs[o];
        const int li = Ls[o];
        const double vp = vi > 0.0 ? vi : 0.0;
        sr[start] = i == 0 ? vp : vp - pw[plen] * pvp;
        cr[start] = vp;                                                          // pw[0] = 1.0
        for (int k = 1; k < li; ++k) cr[start + k] = pw[k] * vp, sr[start + k] = 0.0;
        start += li, plen = li, pvp = vp;
    }
    pools[n] = depth;
}

extern "C" int64_t cwfa_ar1_deconv_workspace_bytes(int N, int T) {
    CWFA_REQUIRE(N >= 0 && T >= 1, CWFA_E_INVAL, "cwfa_ar1_deconv_workspace_bytes: N = %d, T = %d: N >= 0 and T >= 1 are expected", N, T);
    return ((int64_t)N * T * 20 + 7) & ~(int64_t)7;                              // V, W (8 N T each), L (4 N T), a whole number of doubles
}

extern "C" int cwfa_ar1_deconv_f64(const double* y, int N, int T, int64_t stride, double gamma, const double* lam, const double* pw,
                                   double* c, double* s, int32_t* pools, void* ws, void* stream) {
    CWFA_REQUIRE(N >= 0 && T >= 1, CWFA_E_SHAPE, "cwfa_ar1_deconv_f64: N = %d, T = %d: N >= 0 and T >= 1 are expected", N, T);
    CWFA_REQUIRE(pw && ((y && lam && c && s && pools && ws) || N == 0), CWFA_E_INVAL, "cwfa_ar1_deconv_f64: null pointer");
    CWFA_REQUIRE(stride >= T, CWFA_E_INVAL, "cwfa_ar1_deconv_f64: row stride smaller than a row");
    CWFA_REQUIRE(gamma >= 0.0 && gamma < 1.0, CWFA_E_INVAL, "cwfa_ar1_deconv_f64: gamma = %g is not in [0, 1)", gamma);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(lam) | reinterpret_cast<uintptr_t>(pw) |
                   reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(ws)) & 7u) == 0,
                 CWFA_E_ALIGN, "cwfa_ar1_deconv_f64: the float64 arrays and the workspace must be 8-byte aligned");
    if (N == 0) return CWFA_OK;
    const int64_t nt = (int64_t)N * T;
    double* Vs = static_cast<double*>(ws);
    double* Ws = Vs + nt;
    int* Ls = reinterpret_cast<int*>(Ws + nt);
    hipLaunchKernelGGL(ar1_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, y, N, T, stride, gamma, lam, pw, c, s,
                       pools, Vs, Ws, Ls);
    CWFA_LAUNCH_CHECK("cwfa_ar1_deconv_f64");
    return CWFA_OK;
}
