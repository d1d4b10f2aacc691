// Stimulus and seed regression maps: a per-voxel linear regression of a streamed series of volumes against K
// known time courses.  Beside the state of the activity map (neuron_ops.hip) a voxel keeps p[k] = sum of d * r_k, float64, so the maps
// come out of the same single read of every chunk.  Built with -ffp-contract=off: every float64 operation is rounded separately, in
// the order the numpy restatement tests/regress_ref.py repeats.
#include <math.h>
#include "common.h"

typedef double f64x2 __attribute__((ext_vector_type(2)));

// one group of V voxels per thread where there are enough of them, the chip several times over at most (neuron_ops.hip's rule)
static inline int regress_blocks(int64_t units, int threads, int cap) {
    int64_t b = (units + threads - 1) / threads;
    if (b > cap) b = cap;
    return b < 1 ? 1 : (int)b;
}

// ------------------------------------------------------------------------------------------------ the update
// activity_update_kernel's walk -- the same loads, the same operations on x0 / s1 / s2 / vmax / vmin in the same order, so those five
// come out as its bits -- with KB products per voxel and sample added to p[k0 .. k0 + KB).  The rows [T, K] are the same for every
// lane: their index is wave-uniform, so they are read through the scalar cache and enter the multiplications as scalar operands.
// PLAIN = false: the second launch of K > 8, which forms d as the first does and keeps the products only.
template <int V, int KB, bool PLAIN>
__global__ __launch_bounds__(256) void regress_update_kernel(const float* __restrict__ x, float* __restrict__ x0p, double* __restrict__ s1p,
                                                             double* __restrict__ s2p, float* __restrict__ vmaxp, float* __restrict__ vminp,
                                                             double* __restrict__ pp, const double* __restrict__ rows, int T, int K, int k0,
                                                             int64_t groups, int64_t m, int64_t ss, int first) {
    typedef float vec __attribute__((ext_vector_type(V)));
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = g * V;
        const float* p = x + e;
        double* pk = pp + (int64_t)k0 * m + e;
        vec x0, mx, mn;
        double s1[V], s2[V], acc[KB][V];
        if (first) {
            x0 = *reinterpret_cast<const vec*>(p);
            mx = mn = x0;
#pragma unroll
            for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.0;
#pragma unroll
            for (int k = 0; k < KB; ++k)
#pragma unroll
                for (int j = 0; j < V; ++j) acc[k][j] = 0.0;
        } else {
            x0 = *reinterpret_cast<const vec*>(x0p + e);
            if constexpr (PLAIN) {
                mx = *reinterpret_cast<const vec*>(vmaxp + e);
                mn = *reinterpret_cast<const vec*>(vminp + e);
            }
            if constexpr (V == 4) {
                if constexpr (PLAIN) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f64x2 a = *reinterpret_cast<const f64x2*>(s1p + e + 2 * h), b = *reinterpret_cast<const f64x2*>(s2p + e + 2 * h);
                        s1[2 * h] = a[0], s1[2 * h + 1] = a[1], s2[2 * h] = b[0], s2[2 * h + 1] = b[1];
                    }
                }
#pragma unroll
                for (int k = 0; k < KB; ++k)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f64x2 a = *reinterpret_cast<const f64x2*>(pk + k * m + 2 * h);
                        acc[k][2 * h] = a[0], acc[k][2 * h + 1] = a[1];
                    }
            } else {
                if constexpr (PLAIN) s1[0] = s1p[e], s2[0] = s2p[e];
#pragma unroll
                for (int k = 0; k < KB; ++k) acc[k][0] = pk[k * m];
            }
        }
#pragma unroll 2
        for (int s = first ? 1 : 0; s < T; ++s) {
            const vec v = *reinterpret_cast<const vec*>(p + s * ss);
            const double* __restrict__ r = rows + (int64_t)s * K + k0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double d = (double)v[j] - (double)x0[j];
                if constexpr (PLAIN) {
                    s1[j] += d;
                    s2[j] += d * d;
                    mx[j] = (v[j] > mx[j] || v[j] != v[j]) ? v[j] : mx[j];
                    mn[j] = (v[j] < mn[j] || v[j] != v[j]) ? v[j] : mn[j];
                }
#pragma unroll
                for (int k = 0; k < KB; ++k) acc[k][j] += d * r[k];
            }
        }
        if constexpr (PLAIN) {
            if (first) *reinterpret_cast<vec*>(x0p + e) = x0;
            *reinterpret_cast<vec*>(vmaxp + e) = mx;
            *reinterpret_cast<vec*>(vminp + e) = mn;
        }
        if constexpr (V == 4) {
            if constexpr (PLAIN) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    *reinterpret_cast<f64x2*>(s1p + e + 2 * h) = f64x2{s1[2 * h], s1[2 * h + 1]};
                    *reinterpret_cast<f64x2*>(s2p + e + 2 * h) = f64x2{s2[2 * h], s2[2 * h + 1]};
                }
            }
#pragma unroll
            for (int k = 0; k < KB; ++k)
#pragma unroll
                for (int h = 0; h < 2; ++h) *reinterpret_cast<f64x2*>(pk + k * m + 2 * h) = f64x2{acc[k][2 * h], acc[k][2 * h + 1]};
        } else {
            if constexpr (PLAIN) s1p[e] = s1[0], s2p[e] = s2[0];
#pragma unroll
            for (int k = 0; k < KB; ++k) pk[k * m] = acc[k][0];
        }
    }
}

template <int V, bool PLAIN>
static void regress_update_launch(int kb, dim3 grid, hipStream_t st, const float* x, float* x0, double* s1, double* s2, float* vmax,
                                  float* vmin, double* p, const double* rows, int T, int K, int k0, int64_t groups, int64_t m, int64_t ss,
                                  int first) {
#define CWFA_REGRESS_CASE(KB)                                                                                                          \
    case KB:                                                                                                                           \
        hipLaunchKernelGGL((regress_update_kernel<V, KB, PLAIN>), grid, dim3(256), 0, st, x, x0, s1, s2, vmax, vmin, p, rows, T, K, k0, \
                           groups, m, ss, first);                                                                                      \
        break;
    switch (kb) {
        CWFA_REGRESS_CASE(1)
        CWFA_REGRESS_CASE(2)
        CWFA_REGRESS_CASE(3)
        CWFA_REGRESS_CASE(4)
        CWFA_REGRESS_CASE(5)
        CWFA_REGRESS_CASE(6)
        CWFA_REGRESS_CASE(7)
        CWFA_REGRESS_CASE(8)
    }
#undef CWFA_REGRESS_CASE
}

extern "C" int cwfa_activity_update_regress_f32(const float* x, const double* rows, float* x0, double* s1, double* s2, float* vmax,
                                                float* vmin, double* p, int T, int K, int64_t m, int64_t x_ss, int first, void* stream) {
    CWFA_REQUIRE(x && rows && x0 && s1 && s2 && vmax && vmin && p, CWFA_E_INVAL, "cwfa_activity_update_regress_f32: null pointer");
    CWFA_REQUIRE(T >= 0 && m >= 0, CWFA_E_SHAPE, "cwfa_activity_update_regress_f32: negative size");
    CWFA_REQUIRE(K >= 1 && K <= CWFA_REGRESS_MAX_K, CWFA_E_SHAPE, "cwfa_activity_update_regress_f32: 1 .. %d regressors, got %d",
                 CWFA_REGRESS_MAX_K, K);
    CWFA_REQUIRE(first == 0 || first == 1, CWFA_E_INVAL, "cwfa_activity_update_regress_f32: first is 0 or 1");
    CWFA_REQUIRE(!first || T >= 1, CWFA_E_SHAPE, "cwfa_activity_update_regress_f32: the first chunk needs at least one volume");
    CWFA_REQUIRE(T <= 1 || x_ss >= m, CWFA_E_INVAL, "cwfa_activity_update_regress_f32: time stride smaller than a volume");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2) | reinterpret_cast<uintptr_t>(p) |
                   reinterpret_cast<uintptr_t>(rows)) & 7u) == 0,
                 CWFA_E_ALIGN, "cwfa_activity_update_regress_f32: the float64 sums and rows must be 8-byte aligned");
    if (m == 0 || T == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    // with m % 4 == 0 and p on 16 bytes every plane of p starts on 16 bytes
    const bool v4 = (m & 3) == 0 && (T == 1 || (x_ss & 3) == 0) && cwfa_aligned16(x) && cwfa_aligned16(x0) && cwfa_aligned16(s1) &&
                    cwfa_aligned16(s2) && cwfa_aligned16(vmax) && cwfa_aligned16(vmin) && cwfa_aligned16(p);
    const int64_t groups = v4 ? m >> 2 : m;
    const dim3 grid(regress_blocks(groups, 256, 8192));
    // K <= 8: one launch.  Beyond: the first eight with the plain state, then the rest, which only reads x and x0 (in the first
    // chunk x[0], as the first launch does) -- the sums per k are independent, so the split changes no bit
    const int ka = K < 8 ? K : 8;
    if (v4)
        regress_update_launch<4, true>(ka, grid, st, x, x0, s1, s2, vmax, vmin, p, rows, T, K, 0, groups, m, x_ss, first);
    else
        regress_update_launch<1, true>(ka, grid, st, x, x0, s1, s2, vmax, vmin, p, rows, T, K, 0, groups, m, x_ss, first);
    CWFA_LAUNCH_CHECK("cwfa_activity_update_regress_f32");
    if (K > 8) {
        if (v4)
            regress_update_launch<4, false>(K - 8, grid, st, x, x0, s1, s2, vmax, vmin, p, rows, T, K, 8, groups, m, x_ss, first);
        else
            regress_update_launch<1, false>(K - 8, grid, st, x, x0, s1, s2, vmax, vmin, p, rows, T, K, 8, groups, m, x_ss, first);
        CWFA_LAUNCH_CHECK("cwfa_activity_update_regress_f32");
    }
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the regressors' own sums
// Thread k * K + l walks the chunk in time order: Srr[k][l] += r[t][k] * r[t][l]; the threads of column 0 also Sr[k] += r[t][k], and
// thread 0 the row count.  A thread owns its sums, so any chunking gives the same bits.  Over all samples, the first included.
__global__ __launch_bounds__(256) void regress_rows_kernel(const double* __restrict__ rows, int T, int K, double* __restrict__ Sr,
                                                           double* __restrict__ Srr, int64_t* __restrict__ count, int first) {
    const int i = threadIdx.x;
    if (i >= K * K) return;
    const int k = i / K, l = i - k * K;
    double a = first ? 0.0 : Srr[i], b = (l == 0 && !first) ? Sr[k] : 0.0;
    for (int t = 0; t < T; ++t) {
        const double rk = rows[(int64_t)t * K + k], rl = rows[(int64_t)t * K + l];
        a += rk * rl;
        if (l == 0) b += rk;
    }
    Srr[i] = a;
    if (l == 0) Sr[k] = b;
    if (i == 0) *count = (first ? 0 : *count) + T;
}

extern "C" int cwfa_regress_rows_f64(const double* rows, int T, int K, double* Sr, double* Srr, int64_t* count, int first, void* stream) {
    CWFA_REQUIRE(rows && Sr && Srr && count, CWFA_E_INVAL, "cwfa_regress_rows_f64: null pointer");
    CWFA_REQUIRE(T >= 0, CWFA_E_SHAPE, "cwfa_regress_rows_f64: negative size");
    CWFA_REQUIRE(K >= 1 && K <= CWFA_REGRESS_MAX_K, CWFA_E_SHAPE, "cwfa_regress_rows_f64: 1 .. %d regressors, got %d", CWFA_REGRESS_MAX_K, K);
    CWFA_REQUIRE(first == 0 || first == 1, CWFA_E_INVAL, "cwfa_regress_rows_f64: first is 0 or 1");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(Sr) | reinterpret_cast<uintptr_t>(Srr) |
                   reinterpret_cast<uintptr_t>(count)) & 7u) == 0,
                 CWFA_E_ALIGN, "cwfa_regress_rows_f64: rows, sums and count must be 8-byte aligned");
    if (T == 0 && !first) return CWFA_OK;
    hipLaunchKernelGGL(regress_rows_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, rows, T, K, Sr, Srr, count, first);
    CWFA_LAUNCH_CHECK("cwfa_regress_rows_f64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the design: G's diagonal and inverse
// One thread.  G = Srr - Sr Sr' / N (lower triangle), G = L L' row by row, Linv by forward substitution column by column,
// Ginv = Linv' Linv.  status[0]: 0, CWFA_REGRESS_COLLINEAR, CWFA_REGRESS_NONFINITE or CWFA_REGRESS_COUNT; status[1]: the regressor.
__global__ void regress_design_kernel(const double* __restrict__ Sr, const double* __restrict__ Srr, const int64_t* __restrict__ count,
                                      double N, int64_t n_rows, int K, double rcond, double* __restrict__ gdiag, double* __restrict__ ginv,
                                      int* __restrict__ status) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    __shared__ double G[CWFA_REGRESS_MAX_K][CWFA_REGRESS_MAX_K], L[CWFA_REGRESS_MAX_K][CWFA_REGRESS_MAX_K],
        Li[CWFA_REGRESS_MAX_K][CWFA_REGRESS_MAX_K];
    int code = 0, which = 0;
    for (int k = 0; k < K; ++k) gdiag[k] = 0.0;
    for (int i = 0; i < K * K; ++i) ginv[i] = 0.0;
    if (*count != n_rows) code = CWFA_REGRESS_COUNT;
    // the first regressor whose own sums are not finite; failing that (an overflowing product) the first row that holds such an entry
    for (int pass = 0; pass < 2 && !code; ++pass)
        for (int k = 0; k < K && !code; ++k) {
            bool bad = !(fabs(Sr[k]) < INFINITY) || !(fabs(Srr[k * K + k]) < INFINITY);
            for (int l = 0; l < K && pass; ++l) bad = bad || !(fabs(Srr[k * K + l]) < INFINITY);
            if (bad) code = CWFA_REGRESS_NONFINITE, which = k;
        }
    if (!code) {
        for (int k = 0; k < K; ++k)
            for (int l = 0; l <= k; ++l) G[k][l] = Srr[k * K + l] - Sr[k] * Sr[l] / N;
        for (int j = 0; j < K && !code; ++j) {
            double s = G[j][j];
            for (int q = 0; q < j; ++q) s = s - L[j][q] * L[j][q];
            // collinear with the regressors before it, or constant: no variance left beside its own mean square
            if (!(s > rcond * G[j][j]) || !(G[j][j] > rcond * Srr[j * K + j])) {
                code = CWFA_REGRESS_COLLINEAR, which = j;
                break;
            }
            L[j][j] = sqrt(s);
            for (int i = j + 1; i < K; ++i) {
                double u = G[i][j];
                for (int q = 0; q < j; ++q) u = u - L[i][q] * L[j][q];
                L[i][j] = u / L[j][j];
            }
        }
    }
    if (!code) {
        for (int c = 0; c < K; ++c) {
            Li[c][c] = 1.0 / L[c][c];
            for (int i = c + 1; i < K; ++i) {
                double u = 0.0;
                for (int q = c; q < i; ++q) u = u - L[i][q] * Li[q][c];
                Li[i][c] = u / L[i][i];
            }
        }
        for (int k = 0; k < K; ++k) {
            gdiag[k] = G[k][k];
            for (int l = 0; l < K; ++l) {
                double u = 0.0;
                for (int q = (k > l ? k : l); q < K; ++q) u = u + Li[q][k] * Li[q][l];
                ginv[k * K + l] = u;
            }
        }
    }
    status[0] = code, status[1] = which;
}

extern "C" int cwfa_regress_design_f64(const double* Sr, const double* Srr, const int64_t* count, int64_t N, int K, double rcond,
                                       double* gdiag, double* ginv, int* status, void* stream) {
    CWFA_REQUIRE(Sr && Srr && count && gdiag && ginv && status, CWFA_E_INVAL, "cwfa_regress_design_f64: null pointer");
    CWFA_REQUIRE(K >= 1 && K <= CWFA_REGRESS_MAX_K, CWFA_E_SHAPE, "cwfa_regress_design_f64: 1 .. %d regressors, got %d", CWFA_REGRESS_MAX_K, K);
    CWFA_REQUIRE(N >= 1 && N <= 0x7fffffff, CWFA_E_SHAPE, "cwfa_regress_design_f64: needs at least one sample (fewer than 2^31)");
    CWFA_REQUIRE(rcond >= 0.0 && rcond < 1.0, CWFA_E_INVAL, "cwfa_regress_design_f64: rcond is in [0, 1)");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(Sr) | reinterpret_cast<uintptr_t>(Srr) | reinterpret_cast<uintptr_t>(count) |
                   reinterpret_cast<uintptr_t>(gdiag) | reinterpret_cast<uintptr_t>(ginv)) & 7u) == 0 &&
                     (reinterpret_cast<uintptr_t>(status) & 3u) == 0,
                 CWFA_E_ALIGN, "cwfa_regress_design_f64: the float64 tensors and count must be 8-byte aligned, status 4-byte");
    hipLaunchKernelGGL(regress_design_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, Sr, Srr, count, (double)N, N, K, rcond, gdiag, ginv,
                       status);
    CWFA_LAUNCH_CHECK("cwfa_regress_design_f64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the per-voxel finish
// Everything in float64 in the order of DESIGN.md section 34.1, rounded to fp32 at the store.  Sr, gdiag and ginv are indexed by
// compile-time k, l: wave-uniform, read through the scalar cache.
template <int K>
__global__ __launch_bounds__(256) void regress_finish_kernel(const double* __restrict__ s1, const double* __restrict__ s2,
                                                             const double* __restrict__ p, const double* __restrict__ Sr,
                                                             const double* __restrict__ gdiag, const double* __restrict__ ginv, double N,
                                                             double dof, int64_t m, int want, float* __restrict__ corr,
                                                             float* __restrict__ beta, float* __restrict__ tt, float* __restrict__ r2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const double a = s1[i], b = s2[i];
        const double vx = b - a * a / N;
        bool ok = vx > 0.0 && fabs(a) < INFINITY && fabs(b) < INFINITY;
        double c[K], bt[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double pk = p[(int64_t)k * m + i];
            ok = ok && fabs(pk) < INFINITY;
            c[k] = pk - a * Sr[k] / N;
        }
        double fit = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double u = 0.0;
#pragma unroll
            for (int l = 0; l < K; ++l) u = u + ginv[k * K + l] * c[l];
            bt[k] = u;
            fit = fit + c[k] * u;
        }
        const double res = vx - fit, rss = res > 0.0 ? res : 0.0;
        if (want & CWFA_REGRESS_CORR) {
#pragma unroll
            for (int k = 0; k < K; ++k) corr[(int64_t)k * m + i] = ok ? (float)(c[k] / sqrt(vx * gdiag[k])) : 0.f;
        }
        if (want & CWFA_REGRESS_BETA) {
#pragma unroll
            for (int k = 0; k < K; ++k) beta[(int64_t)k * m + i] = ok ? (float)bt[k] : 0.f;
        }
        if (want & CWFA_REGRESS_T) {
            const double s = rss / dof;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double den = sqrt(s * ginv[k * K + k]);
                tt[(int64_t)k * m + i] = (ok && den != 0.0) ? (float)(bt[k] / den) : 0.f;
            }
        }
        if (want & CWFA_REGRESS_R2) r2[i] = ok ? (float)(1.0 - rss / vx) : 0.f;
    }
}

extern "C" int cwfa_regress_finish_f32(const double* s1, const double* s2, const double* p, const double* Sr, const double* gdiag,
                                       const double* ginv, int64_t N, int K, int64_t m, int want, float* corr, float* beta, float* t,
                                       float* r2, void* stream) {
    CWFA_REQUIRE(s1 && s2 && p && Sr && gdiag && ginv, CWFA_E_INVAL, "cwfa_regress_finish_f32: null pointer");
    CWFA_REQUIRE(want > 0 && want < 16, CWFA_E_INVAL, "cwfa_regress_finish_f32: want is a non-empty mask of CWFA_REGRESS_CORR .. R2");
    CWFA_REQUIRE((!(want & CWFA_REGRESS_CORR) || corr) && (!(want & CWFA_REGRESS_BETA) || beta) && (!(want & CWFA_REGRESS_T) || t) &&
                     (!(want & CWFA_REGRESS_R2) || r2),
                 CWFA_E_INVAL, "cwfa_regress_finish_f32: null pointer for a requested output");
    CWFA_REQUIRE(K >= 1 && K <= CWFA_REGRESS_MAX_K, CWFA_E_SHAPE, "cwfa_regress_finish_f32: 1 .. %d regressors, got %d", CWFA_REGRESS_MAX_K, K);
    CWFA_REQUIRE(N >= 1 && N <= 0x7fffffff && m >= 0, CWFA_E_SHAPE,
                 "cwfa_regress_finish_f32: needs at least one sample (fewer than 2^31) and a non-negative size");
    CWFA_REQUIRE(!(want & CWFA_REGRESS_T) || N - K - 1 >= 1, CWFA_E_SHAPE,
                 "cwfa_regress_finish_f32: t needs N - K - 1 >= 1 degrees of freedom, got %lld samples for %d regressors", (long long)N, K);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2) | reinterpret_cast<uintptr_t>(p) |
                   reinterpret_cast<uintptr_t>(Sr) | reinterpret_cast<uintptr_t>(gdiag) | reinterpret_cast<uintptr_t>(ginv)) & 7u) == 0,
                 CWFA_E_ALIGN, "cwfa_regress_finish_f32: the float64 tensors must be 8-byte aligned");
    if (m == 0) return CWFA_OK;
    const dim3 grid(regress_blocks(m, 256, 16384));
    hipStream_t st = (hipStream_t)stream;
    const double Nd = (double)N, dof = (double)(N - K - 1);
#define CWFA_REGRESS_CASE(KK)                                                                                                        \
    case KK:                                                                                                                         \
        hipLaunchKernelGGL(regress_finish_kernel<KK>, grid, dim3(256), 0, st, s1, s2, p, Sr, gdiag, ginv, Nd, dof, m, want, corr, beta, t, \
                           r2);                                                                                                      \
        break;
    switch (K) {
        CWFA_REGRESS_CASE(1)
        CWFA_REGRESS_CASE(2)
        CWFA_REGRESS_CASE(3)
        CWFA_REGRESS_CASE(4)
        CWFA_REGRESS_CASE(5)
        CWFA_REGRESS_CASE(6)
        CWFA_REGRESS_CASE(7)
        CWFA_REGRESS_CASE(8)
        CWFA_REGRESS_CASE(9)
        CWFA_REGRESS_CASE(10)
        CWFA_REGRESS_CASE(11)
        CWFA_REGRESS_CASE(12)
        CWFA_REGRESS_CASE(13)
        CWFA_REGRESS_CASE(14)
        CWFA_REGRESS_CASE(15)
        CWFA_REGRESS_CASE(16)
    }
#undef CWFA_REGRESS_CASE
    CWFA_LAUNCH_CHECK("cwfa_regress_finish_f32");
    return CWFA_OK;
}
