// Neuron detection behind a reconstructed time series: a per-voxel temporal statistic that is accumulated while
// the volumes are produced (the arithmetic of stack_kernel in prep_ops.hip, split over calls), and the 3-D local maxima of a score
// map under a total order on the voxels.  Built with -ffp-contract=off: every fp32 / fp64 operation is rounded separately.
#include <math.h>
#include "common.h"

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long nkey_t;

// one group of V voxels per thread where there are enough of them, the chip several times over at most
static inline int neuron_blocks(int64_t units, int threads, int cap) {
    int64_t b = (units + threads - 1) / threads;
    if (b > cap) b = cap;
    return b < 1 ? 1 : (int)b;
}

// ------------------------------------------------------------------------------------------------ streaming activity map
// State per voxel: x0 (the first sample ever seen), s1 / s2 (float64 sums of d = (double)x - (double)x0 and d * d over the samples after
// the first, in time order), vmax / vmin.  stack_kernel adds the same terms to the same sums in the same order, so mean and std of
// the finish kernel are its bits however the series was cut into chunks.  The maximum propagates NaN like torch.amax.
template <int V>
__global__ __launch_bounds__(256) void activity_update_kernel(const float* __restrict__ x, float* __restrict__ x0p, double* __restrict__ s1p,
                                                              double* __restrict__ s2p, float* __restrict__ vmaxp, float* __restrict__ vminp,
                                                              int T, int64_t groups, int64_t ss, int first) {
    typedef float vec __attribute__((ext_vector_type(V)));
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = g * V;
        const float* p = x + e;
        vec x0, mx, mn;
        double s1[V], s2[V];
        if (first) {
            x0 = *reinterpret_cast<const vec*>(p);
            mx = mn = x0;
#pragma unroll
            for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.0;
        } else {
            x0 = *reinterpret_cast<const vec*>(x0p + e);
            mx = *reinterpret_cast<const vec*>(vmaxp + e);
            mn = *reinterpret_cast<const vec*>(vminp + e);
            if constexpr (V == 4) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f64x2 a = *reinterpret_cast<const f64x2*>(s1p + e + 2 * h), b = *reinterpret_cast<const f64x2*>(s2p + e + 2 * h);
                    s1[2 * h] = a[0], s1[2 * h + 1] = a[1], s2[2 * h] = b[0], s2[2 * h + 1] = b[1];
                }
            } else {
                s1[0] = s1p[e], s2[0] = s2p[e];
            }
        }
#pragma unroll 4
        for (int s = first ? 1 : 0; s < T; ++s) {
            const vec v = *reinterpret_cast<const vec*>(p + s * ss);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double d = (double)v[j] - (double)x0[j];
                s1[j] += d;
                s2[j] += d * d;
                mx[j] = (v[j] > mx[j] || v[j] != v[j]) ? v[j] : mx[j];
                mn[j] = (v[j] < mn[j] || v[j] != v[j]) ? v[j] : mn[j];
            }
        }
        if (first) *reinterpret_cast<vec*>(x0p + e) = x0;
        *reinterpret_cast<vec*>(vmaxp + e) = mx;
        *reinterpret_cast<vec*>(vminp + e) = mn;
        if constexpr (V == 4) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                *reinterpret_cast<f64x2*>(s1p + e + 2 * h) = f64x2{s1[2 * h], s1[2 * h + 1]};
                *reinterpret_cast<f64x2*>(s2p + e + 2 * h) = f64x2{s2[2 * h], s2[2 * h + 1]};
            }
        } else {
            s1p[e] = s1[0], s2p[e] = s2[0];
        }
    }
}

extern "C" int cwfa_activity_update_f32(const float* x, float* x0, double* s1, double* s2, float* vmax, float* vmin, int T, int64_t m,
                                        int64_t x_ss, int first, void* stream) {
    CWFA_REQUIRE(x && x0 && s1 && s2 && vmax && vmin, CWFA_E_INVAL, "cwfa_activity_update_f32: null pointer");
    CWFA_REQUIRE(T >= 0 && m >= 0, CWFA_E_SHAPE, "cwfa_activity_update_f32: negative size");
    CWFA_REQUIRE(first == 0 || first == 1, CWFA_E_INVAL, "cwfa_activity_update_f32: first is 0 or 1");
    CWFA_REQUIRE(!first || T >= 1, CWFA_E_SHAPE, "cwfa_activity_update_f32: the first chunk needs at least one volume");
    CWFA_REQUIRE(T <= 1 || x_ss >= m, CWFA_E_INVAL, "cwfa_activity_update_f32: time stride smaller than a volume");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_activity_update_f32: the float64 sums must be 8-byte aligned");
    if (m == 0 || T == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = (m & 3) == 0 && (T == 1 || (x_ss & 3) == 0) && cwfa_aligned16(x) && cwfa_aligned16(x0) && cwfa_aligned16(s1) &&
                    cwfa_aligned16(s2) && cwfa_aligned16(vmax) && cwfa_aligned16(vmin);
    if (v4)
        hipLaunchKernelGGL(activity_update_kernel<4>, dim3(neuron_blocks(m >> 2, 256, 8192)), dim3(256), 0, st, x, x0, s1, s2, vmax, vmin, T,
                           m >> 2, x_ss, first);
    else
        hipLaunchKernelGGL(activity_update_kernel<1>, dim3(neuron_blocks(m, 256, 8192)), dim3(256), 0, st, x, x0, s1, s2, vmax, vmin, T, m,
                           x_ss, first);
    CWFA_LAUNCH_CHECK("cwfa_activity_update_f32");
    return CWFA_OK;
}

// mean and std by stack_kernel's formulae; the score from the fp32 maps, every operation rounded to fp32
__global__ __launch_bounds__(256) void activity_finish_kernel(const float* __restrict__ x0, const double* __restrict__ s1,
                                                              const double* __restrict__ s2, const float* __restrict__ vmax,
                                                              const float* __restrict__ vmin, double N, int kind, float* __restrict__ mean,
                                                              float* __restrict__ sd, float* __restrict__ score, int64_t m) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const double a = s1[i], b = s2[i];
        const float mo = (float)((double)x0[i] + a / N);
        const double var = (b - a * a / N) / (N - 1.0);
        const float so = (float)sqrt(var < 0.0 ? 0.0 : var);
        float sc;
        switch (kind) {
            case CWFA_ACTIVITY_RANGE: sc = vmax[i] - vmin[i]; break;
            case CWFA_ACTIVITY_PEAK: sc = vmax[i] - mo; break;
            case CWFA_ACTIVITY_SNR: sc = so == 0.f ? 0.f : (vmax[i] - mo) / so; break;
            default: sc = so;
        }
        mean[i] = mo;
        sd[i] = so;
        score[i] = sc;
    }
}

extern "C" int cwfa_activity_finish_f32(const float* x0, const double* s1, const double* s2, const float* vmax, const float* vmin,
                                        int64_t N, int kind, float* mean, float* std, float* score, int64_t m, void* stream) {
    CWFA_REQUIRE(x0 && s1 && s2 && vmax && vmin && mean && std && score, CWFA_E_INVAL, "cwfa_activity_finish_f32: null pointer");
    CWFA_REQUIRE(kind >= CWFA_ACTIVITY_STD && kind <= CWFA_ACTIVITY_SNR, CWFA_E_INVAL, "cwfa_activity_finish_f32: unknown kind %d", kind);
    CWFA_REQUIRE(N >= 1 && N <= 0x7fffffff && m >= 0, CWFA_E_SHAPE,
                 "cwfa_activity_finish_f32: needs at least one sample (fewer than 2^31) and a non-negative size");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_activity_finish_f32: the float64 sums must be 8-byte aligned");
    if (m == 0) return CWFA_OK;
    hipLaunchKernelGGL(activity_finish_kernel, dim3(neuron_blocks(m, 256, 16384)), dim3(256), 0, (hipStream_t)stream, x0, s1, s2, vmax, vmin,
                       (double)N, kind, mean, std, score, m);
    CWFA_LAUNCH_CHECK("cwfa_activity_finish_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ streaming local correlation
// DESIGN.md section 25.  Beside the state above, cc[k][i] = sum over the samples after the first of d_i * d_j, j = i + o_k, for the K
// forward offsets o_k of the neighbourhood: the lexicographically positive half of its (dz, dy, dx), in lexicographic order.  They lie
// in at most five rows of the volume, numbered 0: the voxel's own, 1: y + 1, 2 .. 4: plane z + 1 at y - 1, y, y + 1.
template <int NB>
struct CorrNb {
    static constexpr int K = NB == CWFA_CORR_6 ? 3 : NB == CWFA_CORR_8 ? 4 : 13;
    static constexpr int row(int k) { return k == 0 ? 0 : NB == CWFA_CORR_6 ? (k == 1 ? 1 : 3) : 1 + (k - 1) / 3; }
    static constexpr int dx(int k) { return k == 0 ? 1 : NB == CWFA_CORR_6 ? 0 : (k - 1) % 3 - 1; }
    static constexpr bool uses(int r) { return r <= 1 || NB == CWFA_CORR_26 || (NB == CWFA_CORR_6 && r == 3); }
    static constexpr bool left(int r) { return NB != CWFA_CORR_6 && r != 0; }   // the row is read at x - 1 ..
    static constexpr bool right(int r) { return NB != CWFA_CORR_6 || r == 0; }  // .. and at x + V
};

// A thread owns V voxels of one row (W % V == 0) and keeps, per row it reads, the window x - 1 .. x + V (columns 0 .. V + 1 of w).
// A neighbour's d is formed from its x and x0 as its owner forms it.  In the first chunk every x0 comes from x[0]: the x0 array is
// being written by this launch.  A pair whose neighbour is outside the volume is never added to, so its cc stays the 0.0 of the
// first chunk; its loads are pointed at the thread's own row instead, so that no load stands behind a branch (hipcc puts a wait
// for the load into each such branch, which costs a memory round trip per row and time step).  The grid walks the volume in linear
// order: the rows y + 1 and z + 1 are read by blocks that run at about the same time, so the windows come from L1 / L2 / the
// Infinity Cache.
template <int NB, int V>
__global__ __launch_bounds__(256) void activity_update_corr_kernel(const float* __restrict__ x, float* __restrict__ x0p, double* __restrict__ s1p,
                                                                   double* __restrict__ s2p, float* __restrict__ vmaxp, float* __restrict__ vminp,
                                                                   double* __restrict__ ccp, int T, int D, int H, int W, int64_t ss, int first) {
    typedef float vec __attribute__((ext_vector_type(V)));
    typedef CorrNb<NB> N;
    constexpr int K = N::K;
    const int64_t hw = (int64_t)H * W, m = hw * D, gw = W / V, groups = m / V;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t line = g / gw;
        const int xg = (int)(g - line * gw) * V, y = (int)(line % H), z = (int)(line / H);
        const int64_t e = g * V;
        const bool below = z + 1 < D;
        const bool rv[5] = {true, y + 1 < H, below && y > 0, below, below && y + 1 < H};
        const int64_t ro[5] = {0, rv[1] ? W : 0, rv[2] ? hw - W : 0, rv[3] ? hw : 0, rv[4] ? hw + W : 0};
        const bool lv = xg > 0, rx = xg + V < W;
        const int lo = lv ? -1 : 0, hi = rx ? V : V - 1;
        // the windows of one volume q (at this thread's first voxel): every address is inside the volume
        auto window = [&](const float* q, float (&w)[5][V + 2]) {
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                if (!N::uses(r)) continue;
                const vec t = *reinterpret_cast<const vec*>(q + ro[r]);
#pragma unroll
                for (int j = 0; j < V; ++j) w[r][1 + j] = t[j];
                if (N::left(r)) w[r][0] = q[ro[r] + lo];
                if (N::right(r)) w[r][V + 1] = q[ro[r] + hi];
            }
        };
        const float* p = x + e;
        float b[5][V + 2] = {};
        window(first ? p : x0p + e, b);
        vec mx, mn;
        double s1[V], s2[V], cc[K][V];
        if (first) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                mx[j] = mn[j] = b[0][1 + j];
                s1[j] = s2[j] = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) cc[k][j] = 0.0;
            }
        } else {
            mx = *reinterpret_cast<const vec*>(vmaxp + e);
            mn = *reinterpret_cast<const vec*>(vminp + e);
            if constexpr (V == 1) {
                s1[0] = s1p[e], s2[0] = s2p[e];
#pragma unroll
                for (int k = 0; k < K; ++k) cc[k][0] = ccp[k * m + e];
            } else {
#pragma unroll
                for (int h = 0; h < V / 2; ++h) {
                    const f64x2 a = *reinterpret_cast<const f64x2*>(s1p + e + 2 * h), c = *reinterpret_cast<const f64x2*>(s2p + e + 2 * h);
                    s1[2 * h] = a[0], s1[2 * h + 1] = a[1], s2[2 * h] = c[0], s2[2 * h + 1] = c[1];
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const f64x2 u = *reinterpret_cast<const f64x2*>(ccp + k * m + e + 2 * h);
                        cc[k][2 * h] = u[0], cc[k][2 * h + 1] = u[1];
                    }
                }
            }
        }
#pragma unroll 1
        for (int s = first ? 1 : 0; s < T; ++s) {
            float w[5][V + 2] = {};
            window(p + s * ss, w);
            double d[5][V + 2];
#pragma unroll
            for (int r = 0; r < 5; ++r)
#pragma unroll
                for (int c = 0; c < V + 2; ++c) d[r][c] = (double)w[r][c] - (double)b[r][c];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float v = w[0][1 + j];
                const double di = d[0][1 + j];
                s1[j] += di;
                s2[j] += di * di;
                mx[j] = (v > mx[j] || v != v) ? v : mx[j];
                mn[j] = (v < mn[j] || v != v) ? v : mn[j];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int r = N::row(k), c = 1 + j + N::dx(k);
                    const bool in = rv[r] && (c == 0 ? lv : c == V + 1 ? rx : true);
                    const double sum = cc[k][j] + di * d[r][c];
                    cc[k][j] = in ? sum : cc[k][j];
                }
            }
        }
        if (first) {
            vec x0;
#pragma unroll
            for (int j = 0; j < V; ++j) x0[j] = b[0][1 + j];
            *reinterpret_cast<vec*>(x0p + e) = x0;
        }
        *reinterpret_cast<vec*>(vmaxp + e) = mx;
        *reinterpret_cast<vec*>(vminp + e) = mn;
        if constexpr (V == 1) {
            s1p[e] = s1[0], s2p[e] = s2[0];
#pragma unroll
            for (int k = 0; k < K; ++k) ccp[k * m + e] = cc[k][0];
        } else {
#pragma unroll
            for (int h = 0; h < V / 2; ++h) {
                *reinterpret_cast<f64x2*>(s1p + e + 2 * h) = f64x2{s1[2 * h], s1[2 * h + 1]};
                *reinterpret_cast<f64x2*>(s2p + e + 2 * h) = f64x2{s2[2 * h], s2[2 * h + 1]};
#pragma unroll
                for (int k = 0; k < K; ++k) *reinterpret_cast<f64x2*>(ccp + k * m + e + 2 * h) = f64x2{cc[k][2 * h], cc[k][2 * h + 1]};
            }
        }
    }
}

static inline bool corr_known(int neighbours) { return neighbours == CWFA_CORR_6 || neighbours == CWFA_CORR_8 || neighbours == CWFA_CORR_26; }

// D * H * W without overflow (each factor is below 2^31), -1 where it does not fit 2^40 voxels
static inline int64_t corr_voxels(int D, int H, int W) {
    const int64_t hw = (int64_t)H * W;
    if (D == 0 || hw == 0) return 0;
    return hw > ((int64_t)1 << 40) || D > ((int64_t)1 << 40) / hw ? -1 : hw * D;
}

template <int NB>
static void corr_update_launch(bool v4, hipStream_t st, const float* x, float* x0, double* s1, double* s2, float* vmax, float* vmin, double* cc,
                               int T, int D, int H, int W, int64_t m, int64_t ss, int first) {
    // voxels per thread on the vector path: the (2 + K) float64 sums per voxel are 10 .. 30 registers
    constexpr int V = NB == CWFA_CORR_26 ? 2 : 4;
    if (v4)
        hipLaunchKernelGGL((activity_update_corr_kernel<NB, V>), dim3(neuron_blocks(m / V, 256, 8192)), dim3(256), 0, st, x, x0, s1, s2, vmax, vmin,
                           cc, T, D, H, W, ss, first);
    else
        hipLaunchKernelGGL((activity_update_corr_kernel<NB, 1>), dim3(neuron_blocks(m, 256, 8192)), dim3(256), 0, st, x, x0, s1, s2, vmax, vmin, cc,
                           T, D, H, W, ss, first);
}

extern "C" int cwfa_activity_update_corr_f32(const float* x, float* x0, double* s1, double* s2, float* vmax, float* vmin, double* cc, int T,
                                             int D, int H, int W, int64_t x_ss, int neighbours, int first, void* stream) {
    CWFA_REQUIRE(x && x0 && s1 && s2 && vmax && vmin && cc, CWFA_E_INVAL, "cwfa_activity_update_corr_f32: null pointer");
    CWFA_REQUIRE(T >= 0 && D >= 0 && H >= 0 && W >= 0, CWFA_E_SHAPE, "cwfa_activity_update_corr_f32: negative size");
    const int64_t m = corr_voxels(D, H, W);
    CWFA_REQUIRE(m >= 0, CWFA_E_SHAPE, "cwfa_activity_update_corr_f32: %d x %d x %d voxels are more than 2^40", D, H, W);
    CWFA_REQUIRE(corr_known(neighbours), CWFA_E_INVAL, "cwfa_activity_update_corr_f32: neighbours is 6, 8 or 26, got %d", neighbours);
    CWFA_REQUIRE(first == 0 || first == 1, CWFA_E_INVAL, "cwfa_activity_update_corr_f32: first is 0 or 1");
    CWFA_REQUIRE(!first || T >= 1, CWFA_E_SHAPE, "cwfa_activity_update_corr_f32: the first chunk needs at least one volume");
    CWFA_REQUIRE(T <= 1 || x_ss >= m, CWFA_E_INVAL, "cwfa_activity_update_corr_f32: time stride smaller than a volume");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2) | reinterpret_cast<uintptr_t>(cc)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_activity_update_corr_f32: the float64 sums must be 8-byte aligned");
    if (m == 0 || T == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    // the vector path of cwfa_activity_update_f32, with whole groups inside a row: W, not only D * H * W, is a multiple of 4
    const bool v4 = (W & 3) == 0 && (T == 1 || (x_ss & 3) == 0) && cwfa_aligned16(x) && cwfa_aligned16(x0) && cwfa_aligned16(s1) &&
                    cwfa_aligned16(s2) && cwfa_aligned16(vmax) && cwfa_aligned16(vmin) && cwfa_aligned16(cc);
    if (neighbours == CWFA_CORR_6)
        corr_update_launch<CWFA_CORR_6>(v4, st, x, x0, s1, s2, vmax, vmin, cc, T, D, H, W, m, x_ss, first);
    else if (neighbours == CWFA_CORR_8)
        corr_update_launch<CWFA_CORR_8>(v4, st, x, x0, s1, s2, vmax, vmin, cc, T, D, H, W, m, x_ss, first);
    else
        corr_update_launch<CWFA_CORR_26>(v4, st, x, x0, s1, s2, vmax, vmin, cc, T, D, H, W, m, x_ss, first);
    CWFA_LAUNCH_CHECK("cwfa_activity_update_corr_f32");
    return CWFA_OK;
}

// score_i = (float)(sum of r_ij / n_i) over the in-volume offsets of the whole neighbourhood in lexicographic order: the negatives of
// the forward offsets from the last to the first (the pair's cc is kept at the lower voxel j = i - o_k), then the forward ones.
// r = cov / sqrt(v_i v_j) where that is above 0, else 0: a constant voxel, NaN or inf in a series and N = 1 all give 0, never NaN.
template <int NB>
__global__ __launch_bounds__(256) void activity_corr_finish_kernel(const double* __restrict__ s1, const double* __restrict__ s2,
                                                                   const double* __restrict__ cc, double N, int D, int H, int W,
                                                                   float* __restrict__ score) {
    typedef CorrNb<NB> C;
    constexpr int K = C::K;
    const int64_t hw = (int64_t)H * W, m = hw * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t line = i / W;
        const int xx = (int)(i - line * W), y = (int)(line % H), z = (int)(line / H);
        const double a = s1[i];
        double vi = s2[i] - a * a / N;
        vi = vi < 0.0 ? 0.0 : vi;
        double sum = 0.0;
        int n = 0;
#pragma unroll
        for (int q = 0; q < 2 * K; ++q) {
            const int k = q < K ? K - 1 - q : q - K, sg = q < K ? -1 : 1;
            const int r = C::row(k);
            const int dz = sg * (r >= 2), dy = sg * (r == 0 ? 0 : r == 1 ? 1 : r - 3), dx = sg * C::dx(k);
            const int zz = z + dz, yy = y + dy, xj = xx + dx;
            if (zz < 0 || zz >= D || yy < 0 || yy >= H || xj < 0 || xj >= W) continue;
            const int64_t j = i + dz * hw + (int64_t)dy * W + dx;
            const double c = cc[k * m + (sg < 0 ? j : i)], aj = s1[j];
            double vj = s2[j] - aj * aj / N;
            vj = vj < 0.0 ? 0.0 : vj;
            const double cov = c - a * aj / N, den = sqrt(vi * vj);
            sum += den > 0.0 ? cov / den : 0.0;
            ++n;
        }
        score[i] = n ? (float)(sum / n) : 0.f;
    }
}

extern "C" int cwfa_activity_corr_finish_f32(const double* s1, const double* s2, const double* cc, int64_t N, int D, int H, int W,
                                             int neighbours, float* score, void* stream) {
    CWFA_REQUIRE(s1 && s2 && cc && score, CWFA_E_INVAL, "cwfa_activity_corr_finish_f32: null pointer");
    CWFA_REQUIRE(corr_known(neighbours), CWFA_E_INVAL, "cwfa_activity_corr_finish_f32: neighbours is 6, 8 or 26, got %d", neighbours);
    CWFA_REQUIRE(N >= 1 && N <= 0x7fffffff && D >= 0 && H >= 0 && W >= 0, CWFA_E_SHAPE,
                 "cwfa_activity_corr_finish_f32: needs at least one sample (fewer than 2^31) and non-negative sizes");
    const int64_t m = corr_voxels(D, H, W);
    CWFA_REQUIRE(m >= 0, CWFA_E_SHAPE, "cwfa_activity_corr_finish_f32: %d x %d x %d voxels are more than 2^40", D, H, W);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2) | reinterpret_cast<uintptr_t>(cc)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_activity_corr_finish_f32: the float64 sums must be 8-byte aligned");
    if (m == 0) return CWFA_OK;
    const dim3 grid(neuron_blocks(m, 256, 16384));
    hipStream_t st = (hipStream_t)stream;
    if (neighbours == CWFA_CORR_6)
        hipLaunchKernelGGL(activity_corr_finish_kernel<CWFA_CORR_6>, grid, dim3(256), 0, st, s1, s2, cc, (double)N, D, H, W, score);
    else if (neighbours == CWFA_CORR_8)
        hipLaunchKernelGGL(activity_corr_finish_kernel<CWFA_CORR_8>, grid, dim3(256), 0, st, s1, s2, cc, (double)N, D, H, W, score);
    else
        hipLaunchKernelGGL(activity_corr_finish_kernel<CWFA_CORR_26>, grid, dim3(256), 0, st, s1, s2, cc, (double)N, D, H, W, score);
    CWFA_LAUNCH_CHECK("cwfa_activity_corr_finish_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ 3-D local maxima
// key(v) = ord(S[v]) << 32 | (0xFFFFFFFF - lin(v)): a total order on the voxels, ties on the value going to the lower linear index.
// ord: the order-preserving unsigned image of the fp32 bits after S + 0.0f (-0 and +0 are one value), NaN -> 0.  Outside the volume
// the key is 0, which is below or equal to every key, so a clipped window needs no special case.
__device__ __forceinline__ nkey_t neuron_key(float s, unsigned lin) {
    s = s + 0.0f;
    const unsigned u = __builtin_bit_cast(unsigned, s);
    const unsigned o = s != s ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
    return ((nkey_t)o << 32) | (nkey_t)(0xFFFFFFFFu - lin);
}
__device__ __forceinline__ nkey_t neuron_max(nkey_t a, nkey_t b) { return a > b ? a : b; }

// max of p[0], p[stride], .. p[n * stride] (LDS): four independent reads per step, so their latencies overlap
__device__ __forceinline__ nkey_t neuron_window_max(const nkey_t* p, int stride, int n) {
    nkey_t m = p[0];
    int j = 1;
    for (; j + 3 <= n; j += 4) {
        const nkey_t a = p[j * stride], b = p[(j + 1) * stride], c = p[(j + 2) * stride], d = p[(j + 3) * stride];
        m = neuron_max(neuron_max(m, a), neuron_max(neuron_max(b, c), d));
    }
    for (; j <= n; ++j) m = neuron_max(m, p[j * stride]);
    return m;
}

#define NMAX_TW 64        // output columns of a tile
#define NMAX_THREADS 1024 // 16 waves on a tile: the LDS images allow two blocks per CU, and the walk is bound by LDS latency
#define NMAX_LDS_BYTES 65536
#define NMAX_DEPTH_THREADS 128

// (a) M[z][y][x] = max of the keys over |dy'| <= dy, |dx'| <= dx in plane z.  A block loads the keys of a haloed TH x 64 tile into the
// LDS (A), takes the maximum along x into B, then along y, and writes the 64-bit map.  Tiles are walked by a grid-stride loop.
__global__ __launch_bounds__(NMAX_THREADS) void nmax_plane_kernel(const float* __restrict__ S, nkey_t* __restrict__ M, int H, int W, int dy,
                                                                  int dx, int TH, int64_t tiles, int tiles_x, int tiles_y) {
    extern __shared__ nkey_t nmax_lds[];
    const int AW = NMAX_TW + 2 * dx, AH = TH + 2 * dy;
    nkey_t* A = nmax_lds;
    nkey_t* B = nmax_lds + AH * AW;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tx = (int)(t % tiles_x);
        const int64_t r = t / tiles_x;
        const int ty = (int)(r % tiles_y);
        const int64_t z = r / tiles_y;
        const int y0 = ty * TH, x0 = tx * NMAX_TW;
        const int64_t plane = z * H;
        // a wave per row of the haloed tile, a lane per column: no division by the runtime row length
        for (int yy = threadIdx.x >> 6; yy < AH; yy += NMAX_THREADS / 64) {
            const int gy = y0 + yy - dy;
            for (int xx = threadIdx.x & 63; xx < AW; xx += 64) {
                const int gx = x0 + xx - dx;
                nkey_t k = 0;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    const int64_t lin = (plane + gy) * W + gx;
                    k = neuron_key(S[lin], (unsigned)lin);
                }
                A[yy * AW + xx] = k;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < AH * NMAX_TW; i += NMAX_THREADS) {
            const int yy = i / NMAX_TW, x = i % NMAX_TW;
            B[i] = neuron_window_max(A + yy * AW + x, 1, 2 * dx);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < TH * NMAX_TW; i += NMAX_THREADS) {
            const int y = i / NMAX_TW, x = i % NMAX_TW;
            const int gy = y0 + y, gx = x0 + x;
            if (gy < H && gx < W) M[(plane + gy) * W + gx] = neuron_window_max(B + i, NMAX_TW, 2 * dy);
        }
        // the next tile's load writes A only, and B is not written before every thread has passed the barrier behind that load
    }
}

// (b) a thread owns a pixel and walks z with the last 2 dz + 1 in-plane maxima in its own LDS column (planes outside the volume: 0).
// The window maximum is the key of exactly one voxel: the voxel is a peak iff the index in that key is its own, so S is read for
// those few only.  Peaks are appended as (score bits, linear index) through the one counter, which keeps counting past `capacity`.
__global__ __launch_bounds__(NMAX_DEPTH_THREADS) void nmax_depth_kernel(const float* __restrict__ S, const nkey_t* __restrict__ M, int D, int H,
                                                                        int W, int dz, float thr, int mz, int my, int mx,
                                                                        uint2* __restrict__ out, unsigned long long capacity,
                                                                        unsigned long long* __restrict__ count, int64_t pixels) {
    extern __shared__ nkey_t nmax_lds[];
    const int R = 2 * dz + 1;
    nkey_t* ring = nmax_lds + threadIdx.x;
    for (int64_t p = (int64_t)blockIdx.x * NMAX_DEPTH_THREADS + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * NMAX_DEPTH_THREADS) {
        const int y = (int)(p / W), x = (int)(p % W);
        const bool inside = y >= my && y < H - my && x >= mx && x < W - mx;
        for (int r = 0; r < R; ++r) ring[r * NMAX_DEPTH_THREADS] = 0;
        int slot = 0;
        nkey_t next = M[p];
        for (int zz = 0; zz < D + dz; ++zz) {
            const nkey_t cur = next;
            next = zz + 1 < D ? M[(int64_t)(zz + 1) * pixels + p] : 0;
            ring[slot * NMAX_DEPTH_THREADS] = cur;
            slot = slot + 1 == R ? 0 : slot + 1;
            const int zo = zz - dz;
            if (zo < 0) continue;
            const nkey_t m = neuron_window_max(ring, NMAX_DEPTH_THREADS, R - 1);
            const int64_t lin = (int64_t)zo * pixels + p;
            if (inside && zo >= mz && zo < D - mz && (unsigned)m == 0xFFFFFFFFu - (unsigned)lin) {
                const float s = S[lin];
                if (s == s && s >= thr && neuron_key(s, (unsigned)lin) == m) {
                    const unsigned long long at = atomicAdd(count, 1ull);
                    if (at < capacity) out[at] = uint2{__builtin_bit_cast(unsigned, s), (unsigned)lin};
                }
            }
        }
    }
}

extern "C" int cwfa_local_maxima_f32(const float* score, int D, int H, int W, float thr, int dz, int dy, int dx, int mz, int my, int mx,
                                     void* workspace, void* out, int64_t capacity, int64_t* count, void* stream) {
    CWFA_REQUIRE(count && (score || D == 0 || H == 0 || W == 0), CWFA_E_INVAL, "cwfa_local_maxima_f32: null pointer");
    CWFA_REQUIRE(D >= 0 && H >= 0 && W >= 0, CWFA_E_SHAPE, "cwfa_local_maxima_f32: negative size");
    CWFA_REQUIRE(capacity >= 0 && mz >= 0 && my >= 0 && mx >= 0, CWFA_E_INVAL, "cwfa_local_maxima_f32: negative capacity or margin");
    CWFA_REQUIRE(dz >= 0 && dz <= CWFA_NMAX_MAX_DIST && dy >= 0 && dy <= CWFA_NMAX_MAX_DIST && dx >= 0 && dx <= CWFA_NMAX_MAX_DIST, CWFA_E_SHAPE,
                 "cwfa_local_maxima_f32: half-widths (%d, %d, %d) are not in 0 .. %d", dz, dy, dx, CWFA_NMAX_MAX_DIST);
    // every linear index below 2^32, that is D * H * W <= 2^32, without overflow on the way: each factor is below 2^31
    const int64_t pixels = (int64_t)H * W;
    CWFA_REQUIRE(D == 0 || pixels == 0 || (pixels <= ((int64_t)1 << 32) && (int64_t)D <= ((int64_t)1 << 32) / pixels), CWFA_E_SHAPE,
                 "cwfa_local_maxima_f32: %d x %d x %d voxels do not fit a 32-bit linear index", D, H, W);
    const int64_t n = pixels * D;
    CWFA_REQUIRE(n == 0 || (workspace && (out || capacity == 0)), CWFA_E_INVAL, "cwfa_local_maxima_f32: null pointer");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(count)) & 7u) == 0,
                 CWFA_E_ALIGN, "cwfa_local_maxima_f32: workspace, out and count must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) {
        cwfa_set_error("cwfa_local_maxima_f32: clearing the counter failed");
        return CWFA_E_HIP;
    }
    if (n == 0) return CWFA_OK;
    nkey_t* M = reinterpret_cast<nkey_t*>(workspace);
    // 32 tile rows where the two LDS images fit 64 KiB, 16 otherwise (16 + 32 rows of 96 + 64 keys: 61440 bytes at the largest halo)
    const int row_keys = NMAX_TW + 2 * dx + NMAX_TW;
    const int TH = (int64_t)(32 + 2 * dy) * row_keys * 8 <= NMAX_LDS_BYTES ? 32 : 16;
    const int lds = (TH + 2 * dy) * row_keys * 8;
    const int tiles_x = (W + NMAX_TW - 1) / NMAX_TW, tiles_y = (H + TH - 1) / TH;
    const int64_t tiles = (int64_t)tiles_x * tiles_y * D;
    hipLaunchKernelGGL(nmax_plane_kernel, dim3((unsigned)(tiles < (1 << 20) ? tiles : (1 << 20))), dim3(NMAX_THREADS), lds, st, score, M, H, W, dy,
                       dx, TH, tiles, tiles_x, tiles_y);
    CWFA_LAUNCH_CHECK("cwfa_local_maxima_f32");
    hipLaunchKernelGGL(nmax_depth_kernel, dim3(neuron_blocks(pixels, NMAX_DEPTH_THREADS, 1 << 20)), dim3(NMAX_DEPTH_THREADS),
                       (2 * dz + 1) * NMAX_DEPTH_THREADS * 8, st, score, M, D, H, W, dz, thr, mz, my, mx, reinterpret_cast<uint2*>(out),
                       (unsigned long long)capacity, reinterpret_cast<unsigned long long*>(count), pixels);
    CWFA_LAUNCH_CHECK("cwfa_local_maxima_f32");
    return CWFA_OK;
}
