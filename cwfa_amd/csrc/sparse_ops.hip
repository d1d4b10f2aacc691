// Sparse-activity extraction in front of every other stage: a robust rank-1 background L[t,p] = a[t] * b[p] of a
// frame stack x [T, P] and the thresholded positive residual S = relu(x - L - tau).  b and tau come from per-pixel temporal order
// statistics (tsel_*), a from float64 dot products of every frame with b (fdot_*), S from one elementwise pass (sres_*).
// Built with -ffp-contract=off; the residual is spelled with __fsub_rn / __fmul_rn all the same, so that it stays three roundings
// under any flag.
#include <math.h>
#include <type_traits>
#include "common.h"
#include "conv_internal.h"

// ------------------------------------------------------------------------------------------------ order-preserving keys
// The order of neuron_ops.hip: the unsigned image of the fp32 bits of v + 0.0f, so -0 and +0 are one value (done on the bits: it
// does not depend on the denormal mode).  fp16 values order like their fp32 images, so a stack of fp16 values that is selected
// as it stands gets 16-bit keys of the same construction: half the LDS and half the bisection steps.
__device__ __forceinline__ unsigned tsel_key(float v) {
    unsigned u = __builtin_bit_cast(unsigned, v);
    u = u == 0x80000000u ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tsel_unkey(unsigned k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ unsigned short tsel_key16(unsigned short h) {
    h = (h & 0x7fffu) == 0 ? (unsigned short)0 : h;
    return (h & 0x8000u) ? (unsigned short)~h : (unsigned short)(h | 0x8000u);
}
__device__ __forceinline__ float tsel_unkey16(unsigned k) {
    const unsigned short h = (k & 0x8000u) ? (unsigned short)(k & 0x7fffu) : (unsigned short)~k;
    return (float)__builtin_bit_cast(_Float16, h);
}

struct tsel_ranks {
    int r[4];
};

// the key of element (t, p): KEY = unsigned short reads the fp16 bits as they are; otherwise the value, minus a[t] * b[p] where a
// background is given, in fp32
template <class KEY, bool HALF>
__device__ __forceinline__ KEY tsel_load_key(const void* x, int64_t i, const float* a, int t, float bp) {
    if constexpr (sizeof(KEY) == 2) {
        return tsel_key16(reinterpret_cast<const unsigned short*>(x)[i]);
    } else {
        float v;
        if constexpr (HALF)
            v = (float)reinterpret_cast<const _Float16*>(x)[i];
        else
            v = reinterpret_cast<const float*>(x)[i];
        if (a) v = __fsub_rn(v, __fmul_rn(a[t], bp));
        return tsel_key(v);
    }
}
template <class KEY>
__device__ __forceinline__ float tsel_value(unsigned k) {
    if constexpr (sizeof(KEY) == 2)
        return tsel_unkey16(k);
    else
        return tsel_unkey(k);
}

// ------------------------------------------------------------------------------------------------ the one-read form
// A workgroup owns a tile of 64 pixels (a lane per pixel) and keeps all T keys of the tile in the LDS, 16 bytes per lane and group
// of 4 frames (8 with 16-bit keys): keys[group][64] of 16-byte entries, so a wave reads 64 consecutive entries with one
// ds_read_b128, conflict-free, and counts 4 (8) frames per read.  Wave w owns the groups w, w + 8, ..: it loads them, and it
// counts them, so no barrier stands between a wave's load and its first count, and the waves' loads overlap the others' counting.
// Frames past T in the last group hold the all-ones key, which is below no candidate.  The rank-r value is found from the top bit
// down: with c = #{keys < prefix | bit}, the r-th smallest (from 0) is >= prefix | bit iff c <= r.  Per bit a wave counts its groups
// against the K candidates at once, the waves' counts meet in a double-buffered LDS table (one barrier per bit), and every wave
// adds them up for itself.
//   LDS: 16 KiB of counts + ceil(T / 4) * 1024 bytes (ceil(T / 8) with 16-bit keys).  T = 250: 80896 bytes with 32-bit keys, two
//   workgroups per CU; up to TSEL_LDS_BYTES (one workgroup per CU) the form accepts 144 groups: T <= 576 (1152 with 16-bit keys).
#define TSEL_TILE 64
#define TSEL_WAVES 8
#define TSEL_THREADS (TSEL_TILE * TSEL_WAVES)
#define TSEL_LDS_BYTES 163840
#define TSEL_CNT_WORDS (2 * TSEL_WAVES * 4 * TSEL_TILE)
#define TSEL_GROUP_BYTES (TSEL_TILE * 16)

static inline int tsel_lds_frames(int key_bytes) { return (TSEL_LDS_BYTES - TSEL_CNT_WORDS * 4) / TSEL_GROUP_BYTES * (16 / key_bytes); }

template <int K, class KEY, bool HALF>
__global__ __launch_bounds__(TSEL_THREADS) void tsel_lds_kernel(const void* __restrict__ x, int T, int64_t P, int64_t fs,
                                                                const float* __restrict__ a, const float* __restrict__ b, tsel_ranks rk,
                                                                float* __restrict__ out) {
    constexpr int FPG = 16 / (int)sizeof(KEY);                        // frames per group
    extern __shared__ unsigned tsel_lds[];
    unsigned* cnt = tsel_lds;                                         // [2][TSEL_WAVES][K][64]
    u32x4* keys = reinterpret_cast<u32x4*>(tsel_lds + TSEL_CNT_WORDS); // [G][64]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int G = (T + FPG - 1) / FPG;
    const int64_t p = (int64_t)blockIdx.x * TSEL_TILE + lane;
    const bool live = p < P;
    const int64_t pc = live ? p : P - 1;                              // lanes past the end read the last pixel and write nothing
    const float bp = a ? b[pc] : 0.f;
    constexpr int U = 16 / FPG;                                       // groups per round: 16 rows in flight per wave
    for (int g0 = w; g0 < G; g0 += U * TSEL_WAVES) {
        unsigned k[U][FPG];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < FPG; ++j) {                           // rows past T read row T - 1 and become the all-ones key
                const int t = (g0 + u * TSEL_WAVES) * FPG + j, tc = t < T ? t : T - 1;
                const unsigned key = tsel_load_key<KEY, HALF>(x, (int64_t)tc * fs + pc, a, tc, bp);
                k[u][j] = t < T ? key : (unsigned)(KEY)~(KEY)0;
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int g = g0 + u * TSEL_WAVES;
            if (g >= G) break;
            if constexpr (FPG == 4)
                keys[g * TSEL_TILE + lane] = u32x4{k[u][0], k[u][1], k[u][2], k[u][3]};
            else
                keys[g * TSEL_TILE + lane] = u32x4{k[u][0] | (k[u][1] << 16), k[u][2] | (k[u][3] << 16), k[u][4] | (k[u][5] << 16),
                                                   k[u][6] | (k[u][7] << 16)};
        }
    }

    unsigned prefix[K];
#pragma unroll
    for (int k = 0; k < K; ++k) prefix[k] = 0;
    for (int bit = (int)sizeof(KEY) * 8 - 1; bit >= 0; --bit) {
        unsigned cand[K], c[K];
#pragma unroll
        for (int k = 0; k < K; ++k) cand[k] = prefix[k] | (1u << bit), c[k] = 0;
#pragma unroll 4
        for (int g = w; g < G; g += TSEL_WAVES) {
            const u32x4 v = keys[g * TSEL_TILE + lane];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (FPG == 4) {
#pragma unroll
                    for (int k = 0; k < K; ++k) c[k] += v[i] < cand[k] ? 1u : 0u;
                } else {
                    const unsigned lo = v[i] & 0xffffu, hi = v[i] >> 16;
#pragma unroll
                    for (int k = 0; k < K; ++k) c[k] += (lo < cand[k] ? 1u : 0u) + (hi < cand[k] ? 1u : 0u);
                }
            }
        }
        unsigned* mine = cnt + (bit & 1) * (TSEL_WAVES * K * TSEL_TILE);
#pragma unroll
        for (int k = 0; k < K; ++k) mine[(w * K + k) * TSEL_TILE + lane] = c[k];
        __syncthreads();
        // the table of bit is written again at bit - 2, behind the barrier of bit - 1, which every wave reaches after these reads
#pragma unroll
        for (int k = 0; k < K; ++k) {
            unsigned tot = 0;
#pragma unroll
            for (int ww = 0; ww < TSEL_WAVES; ++ww) tot += mine[(ww * K + k) * TSEL_TILE + lane];
            prefix[k] = tot <= (unsigned)rk.r[k] ? cand[k] : prefix[k];
        }
    }
    if (w == 0 && live) {
#pragma unroll
        for (int k = 0; k < K; ++k) out[(int64_t)k * P + p] = tsel_value<KEY>(prefix[k]);
    }
}

// ------------------------------------------------------------------------------------------------ the streaming form
// Any T: a thread owns a pixel and counts straight from memory, one sweep of the T frames per key bit (16 or 32 reads of the
// stack).  The same keys, the same bisection: the cross-check of the form above, and the path for T beyond its LDS.
template <int K, class KEY, bool HALF>
__global__ __launch_bounds__(256) void tsel_stream_kernel(const void* __restrict__ x, int T, int64_t P, int64_t fs, const float* __restrict__ a,
                                                          const float* __restrict__ b, tsel_ranks rk, float* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x) {
        const float bp = a ? b[p] : 0.f;
        unsigned prefix[K];
#pragma unroll
        for (int k = 0; k < K; ++k) prefix[k] = 0;
        for (int bit = (int)sizeof(KEY) * 8 - 1; bit >= 0; --bit) {
            unsigned cand[K], c[K];
#pragma unroll
            for (int k = 0; k < K; ++k) cand[k] = prefix[k] | (1u << bit), c[k] = 0;
#pragma unroll 4
            for (int t = 0; t < T; ++t) {
                const unsigned key = tsel_load_key<KEY, HALF>(x, (int64_t)t * fs + p, a, t, bp);
#pragma unroll
                for (int k = 0; k < K; ++k) c[k] += key < cand[k] ? 1u : 0u;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) prefix[k] = c[k] <= (unsigned)rk.r[k] ? cand[k] : prefix[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) out[(int64_t)k * P + p] = tsel_value<KEY>(prefix[k]);
    }
}

template <int K, class KEY, bool HALF>
static int tsel_launch(bool lds_form, const void* x, int T, int64_t P, int64_t fs, const float* a, const float* b, const tsel_ranks& rk,
                       float* out, hipStream_t st) {
    if (lds_form) {
        const int lds = TSEL_CNT_WORDS * 4 + (T + 16 / (int)sizeof(KEY) - 1) / (16 / (int)sizeof(KEY)) * TSEL_GROUP_BYTES;
        const int rc = cwfa_max_lds<&tsel_lds_kernel<K, KEY, HALF>>(TSEL_LDS_BYTES, "cwfa_temporal_select");
        if (rc) return rc;
        hipLaunchKernelGGL((tsel_lds_kernel<K, KEY, HALF>), dim3((unsigned)((P + TSEL_TILE - 1) / TSEL_TILE)), dim3(TSEL_THREADS), lds, st, x,
                           T, P, fs, a, b, rk, out);
    } else {
        int64_t blocks = (P + 255) / 256;
        blocks = blocks > (1 << 20) ? (1 << 20) : blocks;
        hipLaunchKernelGGL((tsel_stream_kernel<K, KEY, HALF>), dim3((unsigned)blocks), dim3(256), 0, st, x, T, P, fs, a, b, rk, out);
    }
    CWFA_LAUNCH_CHECK("cwfa_temporal_select");
    return CWFA_OK;
}

template <class KEY, bool HALF>
static int tsel_launch_k(int K, bool lds_form, const void* x, int T, int64_t P, int64_t fs, const float* a, const float* b,
                         const tsel_ranks& rk, float* out, hipStream_t st) {
    switch (K) {
        case 1: return tsel_launch<1, KEY, HALF>(lds_form, x, T, P, fs, a, b, rk, out, st);
        case 2: return tsel_launch<2, KEY, HALF>(lds_form, x, T, P, fs, a, b, rk, out, st);
        case 3: return tsel_launch<3, KEY, HALF>(lds_form, x, T, P, fs, a, b, rk, out, st);
        default: return tsel_launch<4, KEY, HALF>(lds_form, x, T, P, fs, a, b, rk, out, st);
    }
}

extern "C" int cwfa_temporal_select_lds_frames(int dtype, int transformed) {
    CWFA_REQUIRE(dtype == 0 || dtype == 1, CWFA_E_INVAL, "cwfa_temporal_select_lds_frames: dtype is 0 (fp32) or 1 (fp16), got %d", dtype);
    return tsel_lds_frames(dtype == 1 && !transformed ? 2 : 4);
}

extern "C" int cwfa_temporal_select(const void* x, int dtype, int T, int64_t P, int64_t frame_stride, const float* a, const float* b,
                                    const int* ranks, int K, float* out, int form, void* stream) {
    CWFA_REQUIRE(x && ranks && out, CWFA_E_INVAL, "cwfa_temporal_select: null pointer");
    CWFA_REQUIRE(dtype == 0 || dtype == 1, CWFA_E_INVAL, "cwfa_temporal_select: dtype is 0 (fp32) or 1 (fp16), got %d", dtype);
    CWFA_REQUIRE(T >= 0 && P >= 0, CWFA_E_SHAPE, "cwfa_temporal_select: negative size");
    CWFA_REQUIRE((a == nullptr) == (b == nullptr), CWFA_E_INVAL, "cwfa_temporal_select: a and b are given together or not at all");
    CWFA_REQUIRE(K >= 1 && K <= 4, CWFA_E_INVAL, "cwfa_temporal_select: K = %d is not in 1 .. 4", K);
    CWFA_REQUIRE(form >= 0 && form <= 2, CWFA_E_INVAL, "cwfa_temporal_select: unknown form %d", form);
    if (T == 0 || P == 0) return CWFA_OK;
    CWFA_REQUIRE(frame_stride >= P, CWFA_E_INVAL, "cwfa_temporal_select: frame stride smaller than a frame");
    tsel_ranks rk = {{0, 0, 0, 0}};
    for (int k = 0; k < K; ++k) {
        CWFA_REQUIRE(ranks[k] >= 0 && ranks[k] < T, CWFA_E_INVAL, "cwfa_temporal_select: rank %d is not in 0 .. %d", ranks[k], T - 1);
        rk.r[k] = ranks[k];
    }
    const bool key16 = dtype == 1 && !a;
    const int cap = tsel_lds_frames(key16 ? 2 : 4);
    CWFA_REQUIRE(form != 1 || T <= cap, CWFA_E_SHAPE, "cwfa_temporal_select: the one-read form holds at most %d frames, got %d", cap, T);
    CWFA_REQUIRE((P + TSEL_TILE - 1) / TSEL_TILE < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_temporal_select: too many pixels");
    const bool lds_form = form == 1 || (form == 0 && T <= cap);
    hipStream_t st = (hipStream_t)stream;
    if (key16) return tsel_launch_k<unsigned short, true>(K, lds_form, x, T, P, frame_stride, a, b, rk, out, st);
    if (dtype == 1) return tsel_launch_k<unsigned, true>(K, lds_form, x, T, P, frame_stride, a, b, rk, out, st);
    return tsel_launch_k<unsigned, false>(K, lds_form, x, T, P, frame_stride, a, b, rk, out, st);
}

// ------------------------------------------------------------------------------------------------ frame dots
// sums[t] = sum_p x[t,p] * b[p] and sums[T] = sum_p b[p]^2 in float64; a product of two fp32 values is exact there.  A wave owns
// slabs of 1024 pixels (16 per lane, whose b it keeps in registers) and walks the frames of its block's chunk of FDOT_TC frames:
// per frame the lanes' sums meet in a wave sum and lane 0 adds it to the wave's LDS row.  The block adds its four rows in a fixed
// order into ws[block][T + 1]; the finish kernel adds the blocks in ascending order.  Which lane sees which element is a fixed
// function of (T, P) and the launch shape: no atomics, bitwise repeatable.
#define FDOT_WAVES 4
#define FDOT_SLAB 1024
#define FDOT_TC 512
#define FDOT_MAX_BLOCKS 2048

static inline int64_t fdot_blocks(int64_t P) {
    const int64_t slabs = (P + FDOT_SLAB - 1) / FDOT_SLAB;
    int64_t nb = (slabs + FDOT_WAVES - 1) / FDOT_WAVES;
    nb = nb > FDOT_MAX_BLOCKS ? FDOT_MAX_BLOCKS : nb;
    return nb < 1 ? 1 : nb;
}

template <int V, bool HALF>
__global__ __launch_bounds__(64 * FDOT_WAVES) void fdot_kernel(const void* __restrict__ x, int T, int64_t P, int64_t fs, const float* __restrict__ b,
                                                               double* __restrict__ ws, int64_t slabs) {
    typedef float fvec __attribute__((ext_vector_type(V)));
    typedef _Float16 hvec __attribute__((ext_vector_type(V)));
    using xvec = std::conditional_t<HALF, hvec, fvec>;
    using elem = std::conditional_t<HALF, _Float16, float>;
    constexpr int R = 16 / V;
    __shared__ double acc[FDOT_WAVES][FDOT_TC + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t0 = blockIdx.y * FDOT_TC;
    const int tc = T - t0 < FDOT_TC ? T - t0 : FDOT_TC;
    for (int i = threadIdx.x; i < FDOT_WAVES * (FDOT_TC + 1); i += blockDim.x) (&acc[0][0])[i] = 0.0;
    __syncthreads();
    for (int64_t s = (int64_t)blockIdx.x * FDOT_WAVES + w; s < slabs; s += (int64_t)gridDim.x * FDOT_WAVES) {
        int64_t pix[R];
        float bv[R][V];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            pix[r] = s * FDOT_SLAB + (int64_t)(r * 64 + lane) * V;      // V > 1: P is a multiple of V, a group lies inside or outside
            if (pix[r] < P) {
                const fvec v = *reinterpret_cast<const fvec*>(b + pix[r]);
#pragma unroll
                for (int j = 0; j < V; ++j) bv[r][j] = v[j];
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) bv[r][j] = 0.f;
            }
        }
        if (blockIdx.y == 0) {
            double q = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < V; ++j) q += (double)bv[r][j] * (double)bv[r][j];
            q = cwfa_wave_sum(q);
            if (lane == 0) acc[w][FDOT_TC] += q;
        }
        // the next frame's loads are issued before this frame's sum: a wave keeps 2 R loads in flight across its reduction
        xvec cur[R], nxt[R];
        auto load_row = [&](int t, xvec(&v)[R]) {
            const int64_t row = (int64_t)(t0 + t) * fs;
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] = pix[r] < P ? *reinterpret_cast<const xvec*>(reinterpret_cast<const elem*>(x) + row + pix[r]) : xvec{};
        };
        if (tc > 0) load_row(0, cur);
        for (int t = 0; t < tc; ++t) {
            if (t + 1 < tc) load_row(t + 1, nxt);
            double d = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < V; ++j) d += (double)(float)cur[r][j] * (double)bv[r][j];
            d = cwfa_wave_sum(d);
            if (lane == 0) acc[w][t] += d;
#pragma unroll
            for (int r = 0; r < R; ++r) cur[r] = nxt[r];
        }
    }
    __syncthreads();
    double* row = ws + (int64_t)blockIdx.x * ((int64_t)T + 1);
    for (int i = threadIdx.x; i < tc; i += blockDim.x) row[t0 + i] = ((acc[0][i] + acc[1][i]) + acc[2][i]) + acc[3][i];
    if (blockIdx.y == 0 && threadIdx.x == 0) row[T] = ((acc[0][FDOT_TC] + acc[1][FDOT_TC]) + acc[2][FDOT_TC]) + acc[3][FDOT_TC];
}

__global__ __launch_bounds__(256) void fdot_finish_kernel(const double* __restrict__ ws, int nb, int64_t n, int accumulate,
                                                          double* __restrict__ sums) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int i = 0; i < nb; ++i) s += ws[(int64_t)i * n + t];
        sums[t] = accumulate ? sums[t] + s : s;
    }
}

extern "C" int64_t cwfa_frame_dots_workspace_bytes(int T, int64_t P) {
    CWFA_REQUIRE(T >= 0 && P >= 0, CWFA_E_INVAL, "cwfa_frame_dots_workspace_bytes: negative size");
    return P == 0 ? 0 : fdot_blocks(P) * ((int64_t)T + 1) * (int64_t)sizeof(double);
}

extern "C" int cwfa_frame_dots(const void* x, int dtype, int T, int64_t P, int64_t frame_stride, const float* b, double* sums, void* ws,
                               int accumulate, void* stream) {
    CWFA_REQUIRE(sums && ((x && b && ws) || P == 0), CWFA_E_INVAL, "cwfa_frame_dots: null pointer");
    CWFA_REQUIRE(dtype == 0 || dtype == 1, CWFA_E_INVAL, "cwfa_frame_dots: dtype is 0 (fp32) or 1 (fp16), got %d", dtype);
    CWFA_REQUIRE(T >= 0 && P >= 0, CWFA_E_SHAPE, "cwfa_frame_dots: negative size");
    CWFA_REQUIRE(accumulate == 0 || accumulate == 1, CWFA_E_INVAL, "cwfa_frame_dots: accumulate is 0 or 1");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(ws)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_frame_dots: sums and the workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (P == 0) {                                                     // empty: no launch; overwritten sums are zero
        if (!accumulate && hipMemsetAsync(sums, 0, sizeof(double) * ((size_t)T + 1), st) != hipSuccess) {
            cwfa_set_error("cwfa_frame_dots: clearing the sums failed");
            return CWFA_E_HIP;
        }
        return CWFA_OK;
    }
    CWFA_REQUIRE(T <= 1 || frame_stride >= P, CWFA_E_INVAL, "cwfa_frame_dots: frame stride smaller than a frame");
    const int64_t slabs = (P + FDOT_SLAB - 1) / FDOT_SLAB;
    const int nb = (int)fdot_blocks(P);
    const int chunks = T == 0 ? 1 : (int)(((int64_t)T + FDOT_TC - 1) / FDOT_TC);
    CWFA_REQUIRE(chunks <= 65535, CWFA_E_SHAPE, "cwfa_frame_dots: more than %d frames", 65535 * FDOT_TC);
    const dim3 grid(nb, chunks);
    double* slab = static_cast<double*>(ws);
    // 16-byte loads of fp32, 8-byte loads of fp16: four pixels per lane and load, where P, the stride and the bases allow
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x);
    const bool v4 = (P & 3) == 0 && (T <= 1 || (frame_stride & 3) == 0) && cwfa_aligned16(b) && (xa & (dtype ? 7u : 15u)) == 0;
    if (dtype) {
        if (v4) hipLaunchKernelGGL((fdot_kernel<4, true>), grid, dim3(64 * FDOT_WAVES), 0, st, x, T, P, frame_stride, b, slab, slabs);
        else hipLaunchKernelGGL((fdot_kernel<1, true>), grid, dim3(64 * FDOT_WAVES), 0, st, x, T, P, frame_stride, b, slab, slabs);
    } else {
        if (v4) hipLaunchKernelGGL((fdot_kernel<4, false>), grid, dim3(64 * FDOT_WAVES), 0, st, x, T, P, frame_stride, b, slab, slabs);
        else hipLaunchKernelGGL((fdot_kernel<1, false>), grid, dim3(64 * FDOT_WAVES), 0, st, x, T, P, frame_stride, b, slab, slabs);
    }
    CWFA_LAUNCH_CHECK("cwfa_frame_dots");
    const int64_t n = (int64_t)T + 1;
    hipLaunchKernelGGL(fdot_finish_kernel, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0, st, slab, nb, n,
                       accumulate, sums);
    CWFA_LAUNCH_CHECK("cwfa_frame_dots");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the residual
// S = relu(x - a[t] * b[p] - tau[p]), three separately rounded fp32 operations (two without tau); NaN gives 0.  A thread owns V
// pixels, keeps their b and tau, and walks frames blockIdx.y, blockIdx.y + gridDim.y, ..  PAIR: the [T, P, 2] layout, (x, S) per
// pixel, written in the same pass.  x and out may be one fp32 buffer: an element is read before it is written, by the same thread.
template <int V, bool HALF, bool PAIR>
__global__ __launch_bounds__(256) void sres_kernel(const void* x, int T, int64_t P, int64_t fs, const float* __restrict__ a,
                                                   const float* __restrict__ b, const float* __restrict__ tau, float* out) {
    typedef float fvec __attribute__((ext_vector_type(V)));
    typedef _Float16 hvec __attribute__((ext_vector_type(V)));
    const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (p >= P) return;                                               // V > 1: P is a multiple of V
    float bv[V], tv[V];
    {
        const fvec v = *reinterpret_cast<const fvec*>(b + p);
#pragma unroll
        for (int j = 0; j < V; ++j) bv[j] = v[j];
        if (tau) {
            const fvec u = *reinterpret_cast<const fvec*>(tau + p);
#pragma unroll
            for (int j = 0; j < V; ++j) tv[j] = u[j];
        }
    }
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const float at = a[t];
        float xv[V], sv[V];
        if constexpr (HALF) {
            const hvec v = *reinterpret_cast<const hvec*>(reinterpret_cast<const _Float16*>(x) + (int64_t)t * fs + p);
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = (float)v[j];
        } else {
            const fvec v = *reinterpret_cast<const fvec*>(reinterpret_cast<const float*>(x) + (int64_t)t * fs + p);
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = v[j];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float r = __fsub_rn(xv[j], __fmul_rn(at, bv[j]));
            if (tau) r = __fsub_rn(r, tv[j]);
            sv[j] = r > 0.f ? r : 0.f;
        }
        float* o = out + ((int64_t)t * P + p) * (PAIR ? 2 : 1);
        if constexpr (V == 4) {
            if constexpr (PAIR) {
                reinterpret_cast<f32x4*>(o)[0] = f32x4{xv[0], sv[0], xv[1], sv[1]};
                reinterpret_cast<f32x4*>(o)[1] = f32x4{xv[2], sv[2], xv[3], sv[3]};
            } else {
                *reinterpret_cast<f32x4*>(o) = f32x4{sv[0], sv[1], sv[2], sv[3]};
            }
        } else {
            if constexpr (PAIR) o[0] = xv[0], o[1] = sv[0];
            else o[0] = sv[0];
        }
    }
}

extern "C" int cwfa_sparse_residual(const void* x, int dtype, int T, int64_t P, int64_t frame_stride, const float* a, const float* b,
                                    const float* tau, float* out, int pair, void* stream) {
    CWFA_REQUIRE(x && a && b && out, CWFA_E_INVAL, "cwfa_sparse_residual: null pointer");
    CWFA_REQUIRE(dtype == 0 || dtype == 1, CWFA_E_INVAL, "cwfa_sparse_residual: dtype is 0 (fp32) or 1 (fp16), got %d", dtype);
    CWFA_REQUIRE(T >= 0 && P >= 0, CWFA_E_SHAPE, "cwfa_sparse_residual: negative size");
    CWFA_REQUIRE(pair == 0 || pair == 1, CWFA_E_INVAL, "cwfa_sparse_residual: pair is 0 or 1");
    if (T == 0 || P == 0) return CWFA_OK;
    CWFA_REQUIRE(frame_stride >= P, CWFA_E_INVAL, "cwfa_sparse_residual: frame stride smaller than a frame");
    CWFA_REQUIRE(static_cast<const void*>(out) != x || (dtype == 0 && pair == 0 && frame_stride == P), CWFA_E_INVAL,
                 "cwfa_sparse_residual: in place needs an fp32 stack, pair = 0 and a frame stride of P");
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x);
    const bool v4 = (P & 3) == 0 && (frame_stride & 3) == 0 && cwfa_aligned16(b) && (!tau || cwfa_aligned16(tau)) && cwfa_aligned16(out) &&
                    (xa & (dtype ? 7u : 15u)) == 0;
    const int64_t groups = v4 ? P >> 2 : P;
    const int64_t gx = (groups + 255) / 256;
    CWFA_REQUIRE(gx < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_sparse_residual: too many pixels");
    int64_t gy = 8192 / gx < 16 ? 16 : 8192 / gx;                     // enough blocks for the chip, b and tau reused over T / gy frames
    gy = gy > 65535 ? 65535 : gy;
    gy = gy > T ? T : gy;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    hipStream_t st = (hipStream_t)stream;
#define SRES_LAUNCH(V, HALF, PAIR) \
    hipLaunchKernelGGL((sres_kernel<V, HALF, PAIR>), grid, dim3(256), 0, st, x, T, P, frame_stride, a, b, tau, out)
    if (v4) {
        if (dtype) { if (pair) SRES_LAUNCH(4, true, true); else SRES_LAUNCH(4, true, false); }
        else { if (pair) SRES_LAUNCH(4, false, true); else SRES_LAUNCH(4, false, false); }
    } else {
        if (dtype) { if (pair) SRES_LAUNCH(1, true, true); else SRES_LAUNCH(1, true, false); }
        else { if (pair) SRES_LAUNCH(1, false, true); else SRES_LAUNCH(1, false, false); }
    }
#undef SRES_LAUNCH
    CWFA_LAUNCH_CHECK("cwfa_sparse_residual");
    return CWFA_OK;
}
