// Demixing of overlapping footprints: the overlap sums G_nm of the footprints' weights over the intersections of
// their boxes, the mixing coefficients M_nm = (G_nm wsum_m) / (G_mm wsum_n) as the values of a directed CSR structure, and projected
// Gauss-Seidel on F_n = f_n + sum_m M_nm f_m, independently per time step.  Built with -ffp-contract=off: every float64 operation is
// rounded separately, which is what makes coefficients and traces the bits of the numpy restatement.
//
// No kernel indexes with a value the library has not checked.  The pair records of the overlap sums are made here from the checked
// host tables and copied into the caller's workspace on the stream; the CSR index arrays live in a plan (cwfa_demix_plan_create),
// device memory of the library's own that holds what the host check passed.
#include <math.h>
#include <mutex>
#include <unordered_set>
#include <vector>
#include "common.h"

struct DemixPair {           // CWFA_DEMIX_PAIR_BYTES
    int64_t a, b;            // the intersection's first voxel in w, seen from either box
    int nz, ny, nx;          // the intersection
    int a_ny, a_nx, b_ny, b_nx;   // the boxes' own strides
    int pad;
};
static_assert(sizeof(DemixPair) == CWFA_DEMIX_PAIR_BYTES, "cwfa_hip.h states the size of a pair record");

struct cwfa_demix_plan {
    int N, P, filled;
    int64_t E;
    void* block;             // one allocation: val [E] (double), then rowptr [N+1], col, row, pair, diag [E] each, live [N] (int32)
    double* val;
    int32_t *rowptr, *col, *row, *pair, *diag, *live;
};

static std::mutex demix_mutex;
static std::unordered_set<const cwfa_demix_plan*> demix_plans;

static bool demix_known(const cwfa_demix_plan* p) {
    std::lock_guard<std::mutex> g(demix_mutex);
    return p && demix_plans.count(p) != 0;
}

static inline int64_t demix_count(const int32_t* b) { return (int64_t)(b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4]); }

// pairs: 0 <= n <= m < N, strictly ascending in (n, m)
static int demix_check_pairs(const char* fn, const int32_t* pairs, int64_t P, int N) {
    for (int64_t k = 0; k < P; ++k) {
        const int32_t n = pairs[2 * k], m = pairs[2 * k + 1];
        CWFA_REQUIRE(0 <= n && n <= m && m < N, CWFA_E_INVAL, "%s: pair %lld = (%d, %d) is not 0 <= n <= m < %d", fn, (long long)k, n, m, N);
        CWFA_REQUIRE(k == 0 || pairs[2 * k - 2] < n || (pairs[2 * k - 2] == n && pairs[2 * k - 1] < m), CWFA_E_INVAL,
                     "%s: pair %lld = (%d, %d) does not ascend", fn, (long long)k, n, m);
    }
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ overlap sums
// One wave per pair walks the intersection box in its own linear order: lane l adds the voxels l, l + 64, .. in float64 (the product
// of two fp32 weights is exact there), then the butterfly of roi_weighted_sums_kernel.  An empty intersection gives exactly 0.0.
__global__ __launch_bounds__(64) void footprint_overlaps_kernel(const float* __restrict__ w, const DemixPair* __restrict__ pr,
                                                                double* __restrict__ G) {
    const DemixPair q = pr[blockIdx.x];
    const int cnt = q.nz * q.ny * q.nx, plane = q.ny * q.nx;
    const float* wa = w + q.a;
    const float* wb = w + q.b;
    double s = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 64) {
        const int xx = i % q.nx, yy = (i / q.nx) % q.ny, zz = i / plane;
        const double va = (double)wa[((int64_t)zz * q.a_ny + yy) * q.a_nx + xx];
        const double vb = (double)wb[((int64_t)zz * q.b_ny + yy) * q.b_nx + xx];
        s += va * vb;
    }
    s = cwfa_wave_sum(s);
    if (threadIdx.x == 0) G[blockIdx.x] = s;
}

extern "C" int cwfa_footprint_overlaps_f32(const float* w, const int32_t* boxes, const int64_t* offsets, int N, const int32_t* pairs,
                                           int64_t P, void* ws, double* G, void* stream) {
    const char* fn = "cwfa_footprint_overlaps_f32";
    CWFA_REQUIRE(N >= 0 && P >= 0, CWFA_E_SHAPE, "%s: negative size", fn);
    CWFA_REQUIRE(P <= 0x7fffffff, CWFA_E_SHAPE, "%s: 2^31 pairs or more", fn);
    CWFA_REQUIRE(offsets && (boxes || N == 0) && ((pairs && ws && G) || P == 0), CWFA_E_INVAL, "%s: null pointer", fn);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(ws)) & 7u) == 0, CWFA_E_ALIGN,
                 "%s: G and the workspace must be 8-byte aligned", fn);
    CWFA_REQUIRE(offsets[0] == 0, CWFA_E_INVAL, "%s: offsets[0] is %lld, not 0", fn, (long long)offsets[0]);
    for (int i = 0; i < N; ++i) {
        const int32_t* b = boxes + 6 * i;
        CWFA_REQUIRE(0 <= b[0] && b[0] <= b[1] && 0 <= b[2] && b[2] <= b[3] && 0 <= b[4] && b[4] <= b[5], CWFA_E_INVAL,
                     "%s: box %d [%d,%d) x [%d,%d) x [%d,%d) is not a box", fn, i, b[0], b[1], b[2], b[3], b[4], b[5]);
        CWFA_REQUIRE(demix_count(b) < ((int64_t)1 << 31), CWFA_E_SHAPE, "%s: box %d too large", fn, i);
        CWFA_REQUIRE(offsets[i + 1] - offsets[i] == demix_count(b), CWFA_E_INVAL,
                     "%s: offsets[%d + 1] - offsets[%d] = %lld is not the volume of box %d, %lld", fn, i, i,
                     (long long)(offsets[i + 1] - offsets[i]), i, (long long)demix_count(b));
    }
    const int rc = demix_check_pairs(fn, pairs, P, N);
    if (rc != CWFA_OK) return rc;
    CWFA_REQUIRE(w || offsets[N] == 0, CWFA_E_INVAL, "%s: null pointer", fn);
    if (P == 0) return CWFA_OK;
    std::vector<DemixPair> rec((size_t)P);
    for (int64_t k = 0; k < P; ++k) {
        const int32_t n = pairs[2 * k], m = pairs[2 * k + 1];
        const int32_t* a = boxes + 6 * n;
        const int32_t* b = boxes + 6 * m;
        DemixPair& q = rec[(size_t)k];
        int lo[3], len[3];
        bool empty = false;
        for (int d = 0; d < 3; ++d) {
            lo[d] = a[2 * d] > b[2 * d] ? a[2 * d] : b[2 * d];
            const int hi = a[2 * d + 1] < b[2 * d + 1] ? a[2 * d + 1] : b[2 * d + 1];
            len[d] = hi - lo[d];
            empty = empty || len[d] <= 0;
        }
        q.a_ny = a[3] - a[2], q.a_nx = a[5] - a[4], q.b_ny = b[3] - b[2], q.b_nx = b[5] - b[4], q.pad = 0;
        if (empty) {
            q.a = q.b = 0, q.nz = q.ny = q.nx = 0;
            continue;
        }
        q.nz = len[0], q.ny = len[1], q.nx = len[2];
        q.a = offsets[n] + ((int64_t)(lo[0] - a[0]) * q.a_ny + (lo[1] - a[2])) * q.a_nx + (lo[2] - a[4]);
        q.b = offsets[m] + ((int64_t)(lo[0] - b[0]) * q.b_ny + (lo[1] - b[2])) * q.b_nx + (lo[2] - b[4]);
    }
    hipStream_t st = (hipStream_t)stream;
    // the host records live until this returns: the copy is ordered on the stream and waited for
    if (hipMemcpyWithStream(ws, rec.data(), (size_t)P * sizeof(DemixPair), hipMemcpyHostToDevice, st) != hipSuccess) {
        cwfa_set_error("%s: copying the pair records failed", fn);
        return CWFA_E_HIP;
    }
    hipLaunchKernelGGL(footprint_overlaps_kernel, dim3((unsigned)P), dim3(64), 0, st, w, (const DemixPair*)ws, G);
    CWFA_LAUNCH_CHECK(fn);
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the plan
extern "C" int cwfa_demix_plan_create(const int32_t* rowptr, const int32_t* col, int N, const int32_t* pairs, int64_t P,
                                      cwfa_demix_plan** plan) {
    const char* fn = "cwfa_demix_plan_create";
    CWFA_REQUIRE(plan, CWFA_E_INVAL, "%s: null pointer", fn);
    *plan = nullptr;
    CWFA_REQUIRE(N >= 0 && P >= 0, CWFA_E_SHAPE, "%s: negative size", fn);
    CWFA_REQUIRE(P <= 0x7fffffff, CWFA_E_SHAPE, "%s: 2^31 pairs or more", fn);
    CWFA_REQUIRE(rowptr && (pairs || P == 0), CWFA_E_INVAL, "%s: null pointer", fn);
    CWFA_REQUIRE(rowptr[0] == 0, CWFA_E_INVAL, "%s: rowptr[0] is %d, not 0", fn, rowptr[0]);
    for (int n = 0; n < N; ++n)
        CWFA_REQUIRE(rowptr[n + 1] >= rowptr[n], CWFA_E_INVAL, "%s: rowptr decreases at row %d", fn, n);
    const int64_t E = rowptr[N];
    CWFA_REQUIRE(col || E == 0, CWFA_E_INVAL, "%s: null pointer", fn);
    int rc = demix_check_pairs(fn, pairs, P, N);
    if (rc != CWFA_OK) return rc;
    // the diagonal pair of every neuron, then every entry's own pair: the pairs ascend, so a row of them is found by bisection
    std::vector<int32_t> diag_of((size_t)N, -1), host((size_t)(N + 1 + 4 * E + N));
    for (int64_t k = 0; k < P; ++k)
        if (pairs[2 * k] == pairs[2 * k + 1]) diag_of[(size_t)pairs[2 * k]] = (int32_t)k;
    int32_t* h_rowptr = host.data();
    int32_t* h_col = h_rowptr + N + 1;
    int32_t* h_row = h_col + E;
    int32_t* h_pair = h_row + E;
    int32_t* h_diag = h_pair + E;
    for (int n = 0; n <= N; ++n) h_rowptr[n] = rowptr[n];
    for (int n = 0; n < N; ++n)
        for (int64_t e = rowptr[n]; e < rowptr[n + 1]; ++e) {
            const int32_t m = col[e];
            CWFA_REQUIRE(0 <= m && m < N, CWFA_E_INVAL, "%s: column %d of row %d is not in 0 .. %d", fn, m, n, N - 1);
            CWFA_REQUIRE(m != n, CWFA_E_INVAL, "%s: row %d holds its own diagonal", fn, n);
            CWFA_REQUIRE(e == rowptr[n] || col[e - 1] < m, CWFA_E_INVAL, "%s: the columns of row %d do not ascend", fn, n);
            const int32_t lo = n < m ? n : m, hi = n < m ? m : n;
            int64_t l = 0, r = P;
            while (l < r) {
                const int64_t c = (l + r) / 2;
                if (pairs[2 * c] < lo || (pairs[2 * c] == lo && pairs[2 * c + 1] < hi))
                    l = c + 1;
                else
                    r = c;
            }
            CWFA_REQUIRE(l < P && pairs[2 * l] == lo && pairs[2 * l + 1] == hi, CWFA_E_INVAL,
                         "%s: entry (%d, %d) has no pair in the table", fn, n, m);
            CWFA_REQUIRE(diag_of[(size_t)m] >= 0, CWFA_E_INVAL, "%s: the pair table lacks the diagonal pair of neuron %d", fn, m);
            h_col[e] = m, h_row[e] = n, h_pair[e] = (int32_t)l, h_diag[e] = diag_of[(size_t)m];
        }
    cwfa_demix_plan* p = new cwfa_demix_plan();
    p->N = N, p->P = (int)P, p->E = E, p->filled = 0;
    const size_t ints = host.size() * sizeof(int32_t), bytes = (size_t)E * sizeof(double) + ints;
    if (hipMalloc(&p->block, bytes ? bytes : 8) != hipSuccess) {
        delete p;
        cwfa_set_error("%s: allocating %zu device bytes failed", fn, bytes);
        return CWFA_E_HIP;
    }
    p->val = (double*)p->block;
    p->rowptr = (int32_t*)(p->val + E);
    p->col = p->rowptr + N + 1, p->row = p->col + E, p->pair = p->row + E, p->diag = p->pair + E, p->live = p->diag + E;
    if (hipMemcpy(p->rowptr, host.data(), ints, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p->block);
        delete p;
        cwfa_set_error("%s: copying the index arrays failed", fn);
        return CWFA_E_HIP;
    }
    {
        std::lock_guard<std::mutex> g(demix_mutex);
        demix_plans.insert(p);
    }
    *plan = p;
    return CWFA_OK;
}

extern "C" int cwfa_demix_plan_destroy(cwfa_demix_plan* plan) {
    {
        std::lock_guard<std::mutex> g(demix_mutex);
        CWFA_REQUIRE(plan && demix_plans.erase(plan) == 1, CWFA_E_INVAL, "cwfa_demix_plan_destroy: not a live plan");
    }
    const hipError_t e = hipFree(plan->block);
    delete plan;
    if (e != hipSuccess) {
        cwfa_set_error("cwfa_demix_plan_destroy: freeing the plan's device memory failed");
        return CWFA_E_HIP;
    }
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ mixing coefficients
// One thread per entry (n, m): M = (G_nm wsum_m) / (G_mm wsum_n), each operation rounded on its own; 0.0 where G_nm == 0, where
// G_mm, wsum_n or their product is not > 0, and where either footprint is empty.  The first N threads also write live[n].
__global__ __launch_bounds__(256) void demix_coeffs_kernel(const double* __restrict__ G, const double* __restrict__ wsum,
                                                           const int* __restrict__ sizes, const int* __restrict__ row,
                                                           const int* __restrict__ col, const int* __restrict__ pair,
                                                           const int* __restrict__ diag, int64_t E, int N, double* __restrict__ val,
                                                           double* __restrict__ val_out, int* __restrict__ live) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < N) live[e] = sizes[e] > 0 ? 1 : 0;
    if (e >= E) return;
    const int n = row[e], m = col[e];
    const double gnm = G[pair[e]], gmm = G[diag[e]], wn = wsum[n], wm = wsum[m];
    const double num = gnm * wm, den = gmm * wn;
    const bool ok = sizes[n] > 0 && sizes[m] > 0 && gnm != 0.0 && gmm > 0.0 && wn > 0.0 && den > 0.0;
    const double v = ok ? num / den : 0.0;
    val[e] = v;
    if (val_out) val_out[e] = v;
}

extern "C" int cwfa_demix_coeffs_f64(cwfa_demix_plan* plan, const double* G, int64_t P, const double* wsum, const int32_t* sizes,
                                     int N, double* val_out, void* stream) {
    const char* fn = "cwfa_demix_coeffs_f64";
    CWFA_REQUIRE(N >= 0 && P >= 0, CWFA_E_SHAPE, "%s: negative size", fn);
    CWFA_REQUIRE((G || P == 0) && ((wsum && sizes) || N == 0), CWFA_E_INVAL, "%s: null pointer", fn);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(wsum) | reinterpret_cast<uintptr_t>(val_out)) & 7u) == 0,
                 CWFA_E_ALIGN, "%s: the float64 arrays must be 8-byte aligned", fn);
    CWFA_REQUIRE(demix_known(plan), CWFA_E_INVAL, "%s: not a live plan", fn);
    CWFA_REQUIRE(N == plan->N && P == plan->P, CWFA_E_SHAPE, "%s: N = %d, P = %lld, the plan has N = %d, P = %d", fn, N, (long long)P,
                 plan->N, plan->P);
    plan->filled = 1;
    const int64_t units = plan->E > N ? plan->E : N;
    if (units == 0) return CWFA_OK;
    hipLaunchKernelGGL(demix_coeffs_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, wsum, sizes,
                       plan->row, plan->col, plan->pair, plan->diag, plan->E, N, plan->val, val_out, plan->live);
    CWFA_LAUNCH_CHECK(fn);
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ projected Gauss-Seidel
// One thread per time step: it copies its column of F to out and sweeps it in place, n = 0 .. N - 1, the row's entries by ascending
// m.  Lane l of a wave holds step t0 + l, so the 64 reads of f_m and the 64 writes of f_n are one contiguous segment each; rowptr,
// col and val are the same for every lane.  An entry whose coefficient is 0.0 is skipped by selection: its load is issued and its
// product formed, the sum keeps its old value (an empty footprint's NaN reaches nobody).  No thread reads another's column.
// A row's entries are read DEMIX_BATCH at a time and then added in order: taken one by one, every entry waited for two scalar
// loads and a vector load before the next was asked for, and the sweep was bound by that latency.
#define DEMIX_BATCH 8
__global__ __launch_bounds__(64) void demix_solve_kernel(const double* __restrict__ F, int64_t fs, double* __restrict__ out, int N, int T,
                                                         const int* __restrict__ rowptr, const int* __restrict__ col,
                                                         const double* __restrict__ val, const int* __restrict__ live, int n_sweeps,
                                                         double tol, int nonneg, int* __restrict__ sweeps) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    const double* f = F + t;
    double* o = out + t;
    const double nan = __builtin_nan("");
    for (int n = 0; n < N; ++n) o[(int64_t)n * T] = live[n] ? f[(int64_t)n * fs] : nan;
    int k = 0;
    for (;;) {
        bool ok = true;
        for (int n = 0; n < N; ++n) {
            double acc = 0.0;
            for (int e0 = rowptr[n], e1 = rowptr[n + 1]; e0 < e1; e0 += DEMIX_BATCH) {
                double c[DEMIX_BATCH], fm[DEMIX_BATCH];
                int m[DEMIX_BATCH];
#pragma unroll
                for (int j = 0; j < DEMIX_BATCH; ++j) {               // the batch's scalars first, all asked for before one is used
                    const int e = e0 + j < e1 ? e0 + j : e1 - 1;      // past the row's end: its last entry again, coefficient 0.0
                    const double v = val[e];
                    m[j] = col[e];
                    c[j] = e0 + j < e1 ? v : 0.0;
                }
#pragma unroll
                for (int j = 0; j < DEMIX_BATCH; ++j) fm[j] = o[(int64_t)m[j] * T];   // then its loads, all in flight before the first sum
#pragma unroll
                for (int j = 0; j < DEMIX_BATCH; ++j) {
                    const double s = acc + c[j] * fm[j];
                    acc = c[j] != 0.0 ? s : acc;
                }
            }
            const bool alive = live[n] != 0;
            const double fn = alive ? f[(int64_t)n * fs] : nan;
            double nw = fn - acc;
            if (nonneg) nw = nw < 0.0 ? 0.0 : nw;
            nw = nw != nw ? nan : nw;                // one NaN, 0x7ff8000000000000: the sign a subtraction gives a NaN is the machine's
            const double old = o[(int64_t)n * T];
            ok = ok && (!alive || fabs(nw - old) <= tol);   // a NaN change is not <= tol; an empty footprint's row is not iterated
            o[(int64_t)n * T] = nw;
        }
        ++k;
        if (ok || k >= n_sweeps) break;
    }
    sweeps[t] = k;
}

extern "C" int cwfa_demix_solve_f64(const double* F, int64_t f_stride, double* out, int N, int T, const cwfa_demix_plan* plan,
                                    int n_sweeps, double tol, int nonneg, int32_t* sweeps, void* stream) {
    const char* fn = "cwfa_demix_solve_f64";
    CWFA_REQUIRE(N >= 0 && T >= 0, CWFA_E_SHAPE, "%s: negative size", fn);
    CWFA_REQUIRE(n_sweeps >= 1, CWFA_E_INVAL, "%s: n_sweeps = %d is not positive", fn, n_sweeps);
    CWFA_REQUIRE(tol >= 0.0, CWFA_E_INVAL, "%s: tol = %g is negative or NaN", fn, tol);
    CWFA_REQUIRE(nonneg == 0 || nonneg == 1, CWFA_E_INVAL, "%s: nonneg is 0 or 1", fn);
    CWFA_REQUIRE(sweeps || T == 0, CWFA_E_INVAL, "%s: null pointer", fn);
    CWFA_REQUIRE((F && out && F != out) || N == 0 || T == 0, CWFA_E_INVAL, "%s: null pointer, or out is F", fn);
    CWFA_REQUIRE(N <= 1 || f_stride >= T, CWFA_E_INVAL, "%s: row stride smaller than a row", fn);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(F) | reinterpret_cast<uintptr_t>(out)) & 7u) == 0, CWFA_E_ALIGN,
                 "%s: the float64 arrays must be 8-byte aligned", fn);
    CWFA_REQUIRE(demix_known(plan), CWFA_E_INVAL, "%s: not a live plan", fn);
    CWFA_REQUIRE(plan->filled, CWFA_E_INVAL, "%s: the plan has no coefficients yet (cwfa_demix_coeffs_f64)", fn);
    CWFA_REQUIRE(N == plan->N, CWFA_E_SHAPE, "%s: N = %d, the plan has %d neurons", fn, N, plan->N);
    if (T == 0) return CWFA_OK;
    hipLaunchKernelGGL(demix_solve_kernel, dim3((unsigned)(((int64_t)T + 63) / 64)), dim3(64), 0, (hipStream_t)stream, F, f_stride, out, N, T,
                       plan->rowptr, plan->col, plan->val, plan->live, n_sweeps, tol, nonneg, sweeps);
    CWFA_LAUNCH_CHECK(fn);
    return CWFA_OK;
}
