// Neuron footprints behind the detector: an occupancy map of the ROI boxes, weighted box sums and shell sums as
// traces, the streamed float64 statistics of every box voxel against its neuron's seed and neuropil traces, their partial correlation,
// and the footprint as the flood fill of the thresholded correlation from the box's core.  Built with -ffp-contract=off: every float64
// operation is rounded separately, which is what makes the state and the correlation the bits of the numpy restatement.
//
// The box tables are HOST arrays, checked here and handed to the kernels FP_CHUNK neurons at a time in the kernel arguments (the form of
// RoiChunk in eval_ops.hip): what a kernel indexes with is what was checked.  blockIdx.y is the neuron within the chunk.
#include <math.h>
#include "common.h"

#define FP_CHUNK 64
#define FP_SLICE 256          // time steps of the reference traces staged in the LDS at once
#define FP_SELECT_THREADS 1024

struct FpBoxes {
    int box[FP_CHUNK][6];
};
struct FpBoxOffs {
    int box[FP_CHUNK][6];
    int64_t off[FP_CHUNK];
};
struct FpShells {
    int outer[FP_CHUNK][6];
    int inner[FP_CHUNK][6];
};
struct FpOffs {
    int64_t off[FP_CHUNK + 1];
};
struct FpSelect {
    int box[FP_CHUNK][6];
    int core[FP_CHUNK][6];
    int64_t off[FP_CHUNK];
};

static inline int64_t fp_count(const int32_t* b) { return (int64_t)(b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4]); }

// D * H * W without overflow (each factor is below 2^31), -1 where it does not fit 2^40 voxels
static inline int64_t fp_voxels(int D, int H, int W) {
    const int64_t hw = (int64_t)H * W;
    if (D == 0 || hw == 0) return 0;
    return hw > ((int64_t)1 << 40) || D > ((int64_t)1 << 40) / hw ? -1 : hw * D;
}

// every box of the table well-formed, inside the volume and below 2^31 voxels
static int fp_check_boxes(const char* fn, const char* what, const int32_t* boxes, int N, int D, int H, int W) {
    for (int i = 0; i < N; ++i) {
        const int32_t* b = boxes + 6 * i;
        CWFA_REQUIRE(0 <= b[0] && b[0] <= b[1] && b[1] <= D && 0 <= b[2] && b[2] <= b[3] && b[3] <= H && 0 <= b[4] && b[4] <= b[5] && b[5] <= W,
                     CWFA_E_INVAL, "%s: %s %d [%d,%d) x [%d,%d) x [%d,%d) is not inside the %d x %d x %d volume", fn, what, i, b[0], b[1], b[2],
                     b[3], b[4], b[5], D, H, W);
        CWFA_REQUIRE(fp_count(b) < ((int64_t)1 << 31), CWFA_E_SHAPE, "%s: %s %d too large", fn, what, i);
    }
    return CWFA_OK;
}

// offsets[0] = 0 and offsets[n + 1] - offsets[n] = the volume of box n
static int fp_check_offsets(const char* fn, const int32_t* boxes, const int64_t* offsets, int N) {
    CWFA_REQUIRE(offsets[0] == 0, CWFA_E_INVAL, "%s: offsets[0] is %lld, not 0", fn, (long long)offsets[0]);
    for (int i = 0; i < N; ++i)
        CWFA_REQUIRE(offsets[i + 1] - offsets[i] == fp_count(boxes + 6 * i), CWFA_E_INVAL,
                     "%s: offsets[%d + 1] - offsets[%d] = %lld is not the volume of box %d, %lld", fn, i, i,
                     (long long)(offsets[i + 1] - offsets[i]), i, (long long)fp_count(boxes + 6 * i));
    return CWFA_OK;
}

#define FP_CHECK(call)          \
    do {                        \
        const int rc_ = (call); \
        if (rc_ != CWFA_OK) return rc_; \
    } while (0)

static inline unsigned fp_blocks(int64_t units, int threads, int cap) {
    int64_t b = (units + threads - 1) / threads;
    if (b > cap) b = cap;
    return b < 1 ? 1u : (unsigned)b;
}

template <class CK>
static inline int64_t fp_fill_boxes(CK& ck, const int32_t* boxes, int n0, int m) {
    int64_t most = 0;
    for (int i = 0; i < FP_CHUNK; ++i)
        for (int k = 0; k < 6; ++k) ck.box[i][k] = i < m ? boxes[6 * (n0 + i) + k] : 0;
    for (int i = 0; i < m; ++i) most = fp_count(boxes + 6 * (n0 + i)) > most ? fp_count(boxes + 6 * (n0 + i)) : most;
    return most;
}

// ------------------------------------------------------------------------------------------------ occupancy map
__global__ __launch_bounds__(256) void roi_mark_kernel(unsigned char* __restrict__ occ, int H, int W, FpBoxes ck) {
    const int* bx = ck.box[blockIdx.y];
    const int z0 = bx[0], y0 = bx[2], ny = bx[3] - bx[2], x0 = bx[4], nx = bx[5] - bx[4];
    const int cnt = (bx[1] - z0) * ny * nx;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * 256) {
        const int j = (int)i, xx = j % nx, yy = (j / nx) % ny, zz = j / (nx * ny);
        occ[((int64_t)(z0 + zz) * H + y0 + yy) * W + x0 + xx] = 1;   // every writer stores the same byte: overlapping boxes need no order
    }
}

extern "C" int cwfa_roi_mark_u8(const int32_t* boxes, int N, uint8_t* occ, int D, int H, int W, void* stream) {
    CWFA_REQUIRE(D >= 0 && H >= 0 && W >= 0 && N >= 0, CWFA_E_SHAPE, "cwfa_roi_mark_u8: negative size");
    const int64_t m = fp_voxels(D, H, W);
    CWFA_REQUIRE(m >= 0, CWFA_E_SHAPE, "cwfa_roi_mark_u8: %d x %d x %d voxels are more than 2^40", D, H, W);
    CWFA_REQUIRE((occ || m == 0) && (boxes || N == 0), CWFA_E_INVAL, "cwfa_roi_mark_u8: null pointer");
    FP_CHECK(fp_check_boxes("cwfa_roi_mark_u8", "box", boxes, N, D, H, W));
    if (m == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(occ, 0, (size_t)m, st) != hipSuccess) {
        cwfa_set_error("cwfa_roi_mark_u8: clearing the map failed");
        return CWFA_E_HIP;
    }
    for (int n0 = 0; n0 < N; n0 += FP_CHUNK) {
        const int mm = N - n0 < FP_CHUNK ? N - n0 : FP_CHUNK;
        FpBoxes ck;
        const int64_t most = fp_fill_boxes(ck, boxes, n0, mm);
        if (most == 0) continue;
        hipLaunchKernelGGL(roi_mark_kernel, dim3(fp_blocks(most, 256, 4096), mm), dim3(256), 0, st, occ, H, W, ck);
        CWFA_LAUNCH_CHECK("cwfa_roi_mark_u8");
    }
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ weighted box sums
// One wave per (time step, box), the form of roi_means_kernel: lane l adds the voxels l, l + 64, .. of the box's own linear order in
// float64, then the butterfly.  The product of two fp32 values is exact in float64.
template <bool WEIGHTED>
__global__ __launch_bounds__(64) void roi_weighted_sums_kernel(const float* __restrict__ x, int64_t t_stride, int H, int W, FpBoxOffs ck,
                                                               const float* __restrict__ w, double* __restrict__ out, int T) {
    const int t = blockIdx.x;
    const int* bx = ck.box[blockIdx.y];
    const int z0 = bx[0], nz = bx[1] - bx[0], y0 = bx[2], ny = bx[3] - bx[2], x0 = bx[4], nx = bx[5] - bx[4];
    const int cnt = nz * ny * nx;
    const float* p = x + t * t_stride;
    const float* wp = WEIGHTED ? w + ck.off[blockIdx.y] : nullptr;
    double s = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 64) {
        const int xx = i % nx, yy = (i / nx) % ny, zz = i / (nx * ny);
        const double v = (double)p[((int64_t)(z0 + zz) * H + y0 + yy) * W + x0 + xx];
        if constexpr (WEIGHTED)
            s += (double)wp[i] * v;
        else
            s += v;
    }
    s = cwfa_wave_sum(s);
    if (threadIdx.x == 0) out[(int64_t)blockIdx.y * T + t] = s;
}

extern "C" int cwfa_roi_weighted_sums_f32(const float* x, const int32_t* boxes, const int64_t* offsets, const float* w, double* out, int T,
                                          int D, int H, int W, int N, int64_t t_stride, void* stream) {
    CWFA_REQUIRE(x && ((out && boxes) || N == 0) && (!w || offsets), CWFA_E_INVAL, "cwfa_roi_weighted_sums_f32: null pointer");
    CWFA_REQUIRE(T >= 0 && D >= 0 && H >= 0 && W >= 0 && N >= 0, CWFA_E_SHAPE, "cwfa_roi_weighted_sums_f32: negative size");
    const int64_t m = fp_voxels(D, H, W);
    CWFA_REQUIRE(m >= 0, CWFA_E_SHAPE, "cwfa_roi_weighted_sums_f32: %d x %d x %d voxels are more than 2^40", D, H, W);
    CWFA_REQUIRE(T <= 1 || t_stride >= m, CWFA_E_INVAL, "cwfa_roi_weighted_sums_f32: time stride smaller than a volume");
    CWFA_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7u) == 0, CWFA_E_ALIGN, "cwfa_roi_weighted_sums_f32: out must be 8-byte aligned");
    FP_CHECK(fp_check_boxes("cwfa_roi_weighted_sums_f32", "box", boxes, N, D, H, W));
    if (w) FP_CHECK(fp_check_offsets("cwfa_roi_weighted_sums_f32", boxes, offsets, N));
    if (T == 0 || N == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int n0 = 0; n0 < N; n0 += FP_CHUNK) {
        const int mm = N - n0 < FP_CHUNK ? N - n0 : FP_CHUNK;
        FpBoxOffs ck;
        fp_fill_boxes(ck, boxes, n0, mm);
        for (int i = 0; i < FP_CHUNK; ++i) ck.off[i] = w && i < mm ? offsets[n0 + i] : 0;
        if (w)
            hipLaunchKernelGGL(roi_weighted_sums_kernel<true>, dim3(T, mm), dim3(64), 0, st, x, t_stride, H, W, ck, w, out + (int64_t)n0 * T, T);
        else
            hipLaunchKernelGGL(roi_weighted_sums_kernel<false>, dim3(T, mm), dim3(64), 0, st, x, t_stride, H, W, ck, w, out + (int64_t)n0 * T, T);
        CWFA_LAUNCH_CHECK("cwfa_roi_weighted_sums_f32");
    }
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ shell sums
// One workgroup per (time step, neuron) walks the outer box; a voxel counts where it is outside the inner box and its occupancy byte
// is 0.  Both loads are issued for every voxel of the outer box (it lies inside the volume) and the sum takes a selected value: no
// load behind the data-dependent test.
__global__ __launch_bounds__(256) void roi_shell_sums_kernel(const float* __restrict__ x, int64_t t_stride, int H, int W, FpShells ck,
                                                             const unsigned char* __restrict__ occ, double* __restrict__ sums,
                                                             int* __restrict__ counts, int T) {
    __shared__ double red[16];
    const int t = blockIdx.x;
    const int* o = ck.outer[blockIdx.y];
    const int* in = ck.inner[blockIdx.y];
    const int z0 = o[0], y0 = o[2], ny = o[3] - o[2], x0 = o[4], nx = o[5] - o[4];
    const int cnt = (o[1] - z0) * ny * nx;
    const int iz0 = in[0], iz1 = in[1], iy0 = in[2], iy1 = in[3], ix0 = in[4], ix1 = in[5];
    const float* p = x + t * t_stride;
    double s = 0.0;
    int c = 0;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int xx = x0 + i % nx, yy = y0 + (i / nx) % ny, zz = z0 + i / (nx * ny);
        const int64_t lin = ((int64_t)zz * H + yy) * W + xx;
        const float v = p[lin];
        const unsigned char oc = occ[lin];
        const bool inner = zz >= iz0 && zz < iz1 && yy >= iy0 && yy < iy1 && xx >= ix0 && xx < ix1;
        const bool take = !inner && oc == 0;
        s += take ? (double)v : 0.0;
        c += take ? 1 : 0;
    }
    s = cwfa_block_sum(s, red);
    if (threadIdx.x == 0) sums[(int64_t)blockIdx.y * T + t] = s;
    if (t == 0) {
        const double n = cwfa_block_sum((double)c, red);   // below 2^31: exact
        if (threadIdx.x == 0) counts[blockIdx.y] = (int)n;
    }
}

extern "C" int cwfa_roi_shell_sums_f32(const float* x, const int32_t* outer, const int32_t* inner, const uint8_t* occ, double* sums,
                                       int32_t* counts, int T, int D, int H, int W, int N, int64_t t_stride, void* stream) {
    CWFA_REQUIRE(x && occ && ((sums && counts && outer && inner) || N == 0), CWFA_E_INVAL, "cwfa_roi_shell_sums_f32: null pointer");
    CWFA_REQUIRE(T >= 0 && D >= 0 && H >= 0 && W >= 0 && N >= 0, CWFA_E_SHAPE, "cwfa_roi_shell_sums_f32: negative size");
    const int64_t m = fp_voxels(D, H, W);
    CWFA_REQUIRE(m >= 0, CWFA_E_SHAPE, "cwfa_roi_shell_sums_f32: %d x %d x %d voxels are more than 2^40", D, H, W);
    CWFA_REQUIRE(T <= 1 || t_stride >= m, CWFA_E_INVAL, "cwfa_roi_shell_sums_f32: time stride smaller than a volume");
    CWFA_REQUIRE((reinterpret_cast<uintptr_t>(sums) & 7u) == 0, CWFA_E_ALIGN, "cwfa_roi_shell_sums_f32: sums must be 8-byte aligned");
    FP_CHECK(fp_check_boxes("cwfa_roi_shell_sums_f32", "outer box", outer, N, D, H, W));
    FP_CHECK(fp_check_boxes("cwfa_roi_shell_sums_f32", "inner box", inner, N, D, H, W));
    if (T == 0 || N == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int n0 = 0; n0 < N; n0 += FP_CHUNK) {
        const int mm = N - n0 < FP_CHUNK ? N - n0 : FP_CHUNK;
        FpShells ck;
        for (int i = 0; i < FP_CHUNK; ++i)
            for (int k = 0; k < 6; ++k) {
                ck.outer[i][k] = i < mm ? outer[6 * (n0 + i) + k] : 0;
                ck.inner[i][k] = i < mm ? inner[6 * (n0 + i) + k] : 0;
            }
        hipLaunchKernelGGL(roi_shell_sums_kernel, dim3(T, mm), dim3(256), 0, st, x, t_stride, H, W, ck, occ, sums + (int64_t)n0 * T,
                           counts + n0, T);
        CWFA_LAUNCH_CHECK("cwfa_roi_shell_sums_f32");
    }
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ streamed statistics
// State: x0 [V] (the first sample ever seen), acc [4][V] = s1, s2, sc, su, ref [N][7] = c0, u0, e1, e2, g1, g2, eg.  A thread owns one
// state voxel and walks the chunk's time axis; e(t) = c(t) - c0 and g(t) = u(t) - u0 are staged in the LDS FP_SLICE steps at a time.
// The threads past the end of a box walk its last voxel and store nothing, so that no load stands behind a per-lane test.  Thread 0 of
// a neuron's first block adds the neuron's own five sums.  c, u and ref arrive advanced to the chunk's first neuron.
template <bool NP>
__global__ __launch_bounds__(256) void footprint_update_kernel(const float* __restrict__ x, int64_t ss, int H, int W, FpBoxOffs ck,
                                                               const double* __restrict__ c, const double* __restrict__ u,
                                                               float* __restrict__ x0p, double* __restrict__ acc, double* __restrict__ ref,
                                                               int T, int64_t V, int first) {
    __shared__ double es[FP_SLICE], gs[NP ? FP_SLICE : 1];
    const int n = blockIdx.y;
    const int* bx = ck.box[n];
    const int z0 = bx[0], y0 = bx[2], ny = bx[3] - bx[2], x0 = bx[4], nx = bx[5] - bx[4];
    const int cnt = (bx[1] - z0) * ny * nx;
    const double* cn = c + (int64_t)n * T;
    const double* un = NP ? u + (int64_t)n * T : nullptr;
    double* rn = ref + (int64_t)n * 7;
    const double c0 = first ? cn[0] : rn[0];
    double u0 = 0.0;
    if constexpr (NP) u0 = first ? un[0] : rn[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double e1 = 0.0, e2 = 0.0, g1 = 0.0, g2 = 0.0, eg = 0.0;
        if (!first) e1 = rn[2], e2 = rn[3], g1 = rn[4], g2 = rn[5], eg = rn[6];
        for (int s = first ? 1 : 0; s < T; ++s) {
            const double e = cn[s] - c0;
            e1 += e;
            e2 += e * e;
            if constexpr (NP) {
                const double g = un[s] - u0;
                g1 += g;
                g2 += g * g;
                eg += e * g;
            }
        }
        if (first) rn[0] = c0, rn[1] = u0;
        rn[2] = e1, rn[3] = e2, rn[4] = g1, rn[5] = g2, rn[6] = eg;
    }
    if ((int64_t)blockIdx.x * 256 >= cnt) return;   // the whole block: an empty box, or a box shorter than the chunk's longest
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool own = i < cnt;
    const int ii = own ? i : cnt - 1;
    const int xx = ii % nx, yy = (ii / nx) % ny, zz = ii / (nx * ny);
    const float* p = x + ((int64_t)(z0 + zz) * H + y0 + yy) * W + x0 + xx;
    const int64_t v = ck.off[n] + ii;
    float xf;
    double s1, s2, sc, su;
    if (first) {
        xf = p[0];
        s1 = s2 = sc = su = 0.0;
    } else {
        xf = x0p[v];
        s1 = acc[v], s2 = acc[V + v], sc = acc[2 * V + v], su = acc[3 * V + v];
    }
    const double xd = (double)xf;
    for (int t0 = first ? 1 : 0; t0 < T; t0 += FP_SLICE) {
        const int len = T - t0 < FP_SLICE ? T - t0 : FP_SLICE;
        __syncthreads();
        for (int j = threadIdx.x; j < len; j += 256) {
            es[j] = cn[t0 + j] - c0;
            if constexpr (NP) gs[j] = un[t0 + j] - u0;
        }
        __syncthreads();
        const float* q = p + (int64_t)t0 * ss;
#pragma unroll 4
        for (int j = 0; j < len; ++j) {
            const double d = (double)q[(int64_t)j * ss] - xd;
            s1 += d;
            s2 += d * d;
            sc += d * es[j];
            if constexpr (NP) su += d * gs[j];
        }
    }
    if (own) {
        if (first) x0p[v] = xf;
        acc[v] = s1, acc[V + v] = s2, acc[2 * V + v] = sc, acc[3 * V + v] = su;
    }
}

extern "C" int cwfa_footprint_update_f32(const float* x, const int32_t* boxes, const int64_t* offsets, const double* c, const double* u,
                                         float* x0, double* acc, double* ref, int T, int D, int H, int W, int N, int64_t t_stride, int first,
                                         void* stream) {
    CWFA_REQUIRE(x && offsets && ((boxes && c && ref) || N == 0), CWFA_E_INVAL, "cwfa_footprint_update_f32: null pointer");
    CWFA_REQUIRE(T >= 0 && D >= 0 && H >= 0 && W >= 0 && N >= 0, CWFA_E_SHAPE, "cwfa_footprint_update_f32: negative size");
    const int64_t m = fp_voxels(D, H, W);
    CWFA_REQUIRE(m >= 0, CWFA_E_SHAPE, "cwfa_footprint_update_f32: %d x %d x %d voxels are more than 2^40", D, H, W);
    CWFA_REQUIRE(first == 0 || first == 1, CWFA_E_INVAL, "cwfa_footprint_update_f32: first is 0 or 1");
    CWFA_REQUIRE(!first || T >= 1, CWFA_E_SHAPE, "cwfa_footprint_update_f32: the first chunk needs at least one volume");
    CWFA_REQUIRE(T <= 1 || t_stride >= m, CWFA_E_INVAL, "cwfa_footprint_update_f32: time stride smaller than a volume");
    FP_CHECK(fp_check_boxes("cwfa_footprint_update_f32", "box", boxes, N, D, H, W));
    FP_CHECK(fp_check_offsets("cwfa_footprint_update_f32", boxes, offsets, N));
    const int64_t V = offsets[N];
    CWFA_REQUIRE((x0 && acc) || V == 0, CWFA_E_INVAL, "cwfa_footprint_update_f32: null pointer");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(acc) |
                   reinterpret_cast<uintptr_t>(ref)) & 7u) == 0,
                 CWFA_E_ALIGN, "cwfa_footprint_update_f32: the float64 arrays must be 8-byte aligned");
    if (T == 0 || N == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int n0 = 0; n0 < N; n0 += FP_CHUNK) {
        const int mm = N - n0 < FP_CHUNK ? N - n0 : FP_CHUNK;
        FpBoxOffs ck;
        const int64_t most = fp_fill_boxes(ck, boxes, n0, mm);
        for (int i = 0; i < FP_CHUNK; ++i) ck.off[i] = i < mm ? offsets[n0 + i] : 0;
        const dim3 grid(fp_blocks(most, 256, 1 << 23), mm);
        const double* cc = c + (int64_t)n0 * T;
        double* rr = ref + (int64_t)n0 * 7;
        if (u)
            hipLaunchKernelGGL(footprint_update_kernel<true>, grid, dim3(256), 0, st, x, t_stride, H, W, ck, cc, u + (int64_t)n0 * T, x0, acc, rr,
                               T, V, first);
        else
            hipLaunchKernelGGL(footprint_update_kernel<false>, grid, dim3(256), 0, st, x, t_stride, H, W, ck, cc, u, x0, acc, rr, T, V, first);
        CWFA_LAUNCH_CHECK("cwfa_footprint_update_f32");
    }
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ partial correlation
// r = den > 0 ? cov / den : 0 with den = sqrt(v_a v_b): a constant series, NaN or inf anywhere and T = 1 make den 0 or NaN, so r = 0.
__device__ __forceinline__ double fp_var(double s1, double s2, double T) {
    const double v = s2 - s1 * s1 / T;
    return v < 0.0 ? 0.0 : v;
}
__device__ __forceinline__ double fp_r(double sab, double sa, double sb, double va, double vb, double T) {
    const double den = sqrt(va * vb), cov = sab - sa * sb / T;
    return den > 0.0 ? cov / den : 0.0;
}

__global__ __launch_bounds__(256) void footprint_corr_kernel(const double* __restrict__ acc, const double* __restrict__ ref, FpOffs ck,
                                                             int64_t V, double T, int neuropil, float* __restrict__ corr) {
    const int n = blockIdx.y;
    const int64_t o = ck.off[n], cnt = ck.off[n + 1] - o;
    const double* rn = ref + (int64_t)n * 7;
    const double e1 = rn[2], e2 = rn[3], g1 = rn[4], g2 = rn[5], eg = rn[6];
    const double ve = fp_var(e1, e2, T), vg = fp_var(g1, g2, T);
    const double reg = fp_r(eg, e1, g1, ve, vg, T);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * 256) {
        const int64_t v = o + i;
        const double s1 = acc[v], s2 = acc[V + v], sc = acc[2 * V + v], su = acc[3 * V + v];
        const double vi = fp_var(s1, s2, T);
        const double rie = fp_r(sc, s1, e1, vi, ve, T);
        double r = rie;
        if (neuropil) {
            const double rig = fp_r(su, s1, g1, vi, vg, T);
            const double q = (1.0 - rig * rig) * (1.0 - reg * reg);
            r = q > 0.0 ? (rie - rig * reg) / sqrt(q) : 0.0;
        }
        corr[v] = (float)r;
    }
}

extern "C" int cwfa_footprint_corr_f32(const double* acc, const double* ref, const int64_t* offsets, int N, int64_t T, int neuropil,
                                       float* corr, void* stream) {
    CWFA_REQUIRE(offsets && (ref || N == 0), CWFA_E_INVAL, "cwfa_footprint_corr_f32: null pointer");
    CWFA_REQUIRE(N >= 0, CWFA_E_SHAPE, "cwfa_footprint_corr_f32: negative size");
    CWFA_REQUIRE(T >= 1 && T <= 0x7fffffff, CWFA_E_SHAPE, "cwfa_footprint_corr_f32: needs at least one sample (fewer than 2^31)");
    CWFA_REQUIRE(neuropil == 0 || neuropil == 1, CWFA_E_INVAL, "cwfa_footprint_corr_f32: neuropil is 0 or 1");
    CWFA_REQUIRE(offsets[0] == 0, CWFA_E_INVAL, "cwfa_footprint_corr_f32: offsets[0] is %lld, not 0", (long long)offsets[0]);
    for (int i = 0; i < N; ++i)
        CWFA_REQUIRE(offsets[i + 1] >= offsets[i], CWFA_E_INVAL, "cwfa_footprint_corr_f32: offsets decrease at %d", i);
    const int64_t V = offsets[N];
    CWFA_REQUIRE((acc && corr) || V == 0, CWFA_E_INVAL, "cwfa_footprint_corr_f32: null pointer");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(ref)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_footprint_corr_f32: the float64 arrays must be 8-byte aligned");
    if (V == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int n0 = 0; n0 < N; n0 += FP_CHUNK) {
        const int mm = N - n0 < FP_CHUNK ? N - n0 : FP_CHUNK;
        FpOffs ck;
        int64_t most = 0;
        for (int i = 0; i <= FP_CHUNK; ++i) ck.off[i] = offsets[n0 + (i < mm ? i : mm)];
        for (int i = 0; i < mm; ++i) most = ck.off[i + 1] - ck.off[i] > most ? ck.off[i + 1] - ck.off[i] : most;
        if (most == 0) continue;
        hipLaunchKernelGGL(footprint_corr_kernel, dim3(fp_blocks(most, 256, 4096), mm), dim3(256), 0, st, acc, ref + (int64_t)n0 * 7, ck, V,
                           (double)T, neuropil, corr);
        CWFA_LAUNCH_CHECK("cwfa_footprint_corr_f32");
    }
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ footprint selection
// One workgroup per neuron.  A byte per box voxel in the LDS: bit 0 = above (corr >= thr), bit 1 = in the footprint; the footprint
// starts as the above voxels of the core.  A sweep: every thread forms, for the voxels it owns (i = thread, thread + 1024, ..: at most
// 32 of them, one bit each), "above, not yet in, and a face neighbour inside the box is in" from the bytes as they stand; behind a
// barrier it sets those bytes.  A sweep that sets nothing ends the fill.  The set only grows and is bounded by the connected component,
// so the fixpoint is the component whatever the sweep order.  Wave 0 then adds the weights in the box's linear order from 0.0.
__global__ __launch_bounds__(FP_SELECT_THREADS) void footprint_select_kernel(const float* __restrict__ corr, FpSelect ck, float thr,
                                                                             float* __restrict__ w, double* __restrict__ wsum,
                                                                             int* __restrict__ size) {
    extern __shared__ unsigned char fp_lds[];
    __shared__ int part[FP_SELECT_THREADS / 64];
    const int n = blockIdx.x;
    const int* bx = ck.box[n];
    const int* co = ck.core[n];
    const int ny = bx[3] - bx[2], nx = bx[5] - bx[4], nz = bx[1] - bx[0];
    const int plane = ny * nx, cnt = nz * plane;
    const int cz0 = co[0] - bx[0], cz1 = co[1] - bx[0], cy0 = co[2] - bx[2], cy1 = co[3] - bx[2], cx0 = co[4] - bx[4], cx1 = co[5] - bx[4];
    const float* cp = corr + ck.off[n];
    float* wp = w + ck.off[n];
    for (int i = threadIdx.x; i < cnt; i += FP_SELECT_THREADS) {
        const int xx = i % nx, yy = (i / nx) % ny, zz = i / plane;
        const bool above = cp[i] >= thr;
        const bool core = zz >= cz0 && zz < cz1 && yy >= cy0 && yy < cy1 && xx >= cx0 && xx < cx1;
        fp_lds[i] = above ? (core ? 3 : 1) : 0;
    }
    __syncthreads();
    for (;;) {
        unsigned grow = 0;
        int k = 0;
        for (int i = threadIdx.x; i < cnt; i += FP_SELECT_THREADS, ++k) {
            const int xx = i % nx, yy = (i / nx) % ny, zz = i / plane;
            // a neighbour outside the box reads the voxel's own byte, which is not "in" where it matters
            const unsigned near = fp_lds[xx > 0 ? i - 1 : i] | fp_lds[xx + 1 < nx ? i + 1 : i] | fp_lds[yy > 0 ? i - nx : i] |
                                  fp_lds[yy + 1 < ny ? i + nx : i] | fp_lds[zz > 0 ? i - plane : i] | fp_lds[zz + 1 < nz ? i + plane : i];
            grow |= (fp_lds[i] == 1 && (near & 2)) ? 1u << k : 0u;
        }
        __syncthreads();
        k = 0;
        for (int i = threadIdx.x; i < cnt; i += FP_SELECT_THREADS, ++k)
            if (grow >> k & 1) fp_lds[i] = 3;
        if (!__syncthreads_or(grow != 0)) break;
    }
    int mine = 0;
    for (int i = threadIdx.x; i < cnt; i += FP_SELECT_THREADS) {
        const bool in = fp_lds[i] == 3;
        wp[i] = in ? cp[i] : 0.f;
        mine += in ? 1 : 0;
    }
    // the size: a wave sum, then the sixteen partial counts; the weights' sum: wave 0, which still reads the bytes
    const int ws = (int)cwfa_wave_sum((float)mine);   // at most 32 * 64: exact in fp32
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ws;
    __syncthreads();
    if (threadIdx.x < 64) {
        double sum = 0.0;
        for (int b = 0; b < cnt; b += 64) {
            const int i = b + threadIdx.x;
            const float mineval = i < cnt && fp_lds[i] == 3 ? cp[i] : 0.f;   // 64 loads in flight, then the serial additions
            const int len = cnt - b < 64 ? cnt - b : 64;
            for (int j = 0; j < len; ++j) sum += (double)__shfl(mineval, j, 64);
        }
        if (threadIdx.x == 0) {
            int total = 0;
            for (int j = 0; j < FP_SELECT_THREADS / 64; ++j) total += part[j];
            wsum[n] = sum;
            size[n] = total;
        }
    }
}

extern "C" int cwfa_footprint_select_f32(const float* corr, const int32_t* boxes, const int32_t* cores, const int64_t* offsets, int N,
                                         float thr, float* w, double* wsum, int32_t* size, void* stream) {
    CWFA_REQUIRE(offsets && ((boxes && cores && wsum && size) || N == 0), CWFA_E_INVAL, "cwfa_footprint_select_f32: null pointer");
    CWFA_REQUIRE(N >= 0, CWFA_E_SHAPE, "cwfa_footprint_select_f32: negative size");
    CWFA_REQUIRE(thr > 0.f && thr <= 1.f, CWFA_E_INVAL, "cwfa_footprint_select_f32: thr = %g is not in (0, 1]", (double)thr);
    for (int i = 0; i < N; ++i) {
        const int32_t* b = boxes + 6 * i;
        const int32_t* c = cores + 6 * i;
        CWFA_REQUIRE(0 <= b[0] && b[0] <= b[1] && 0 <= b[2] && b[2] <= b[3] && 0 <= b[4] && b[4] <= b[5], CWFA_E_INVAL,
                     "cwfa_footprint_select_f32: box %d [%d,%d) x [%d,%d) x [%d,%d) is not a box", i, b[0], b[1], b[2], b[3], b[4], b[5]);
        CWFA_REQUIRE(fp_count(b) <= CWFA_FOOTPRINT_SELECT_MAX, CWFA_E_SHAPE, "cwfa_footprint_select_f32: box %d has %lld voxels, more than 2^15", i,
                     (long long)fp_count(b));
        CWFA_REQUIRE(b[0] <= c[0] && c[0] <= c[1] && c[1] <= b[1] && b[2] <= c[2] && c[2] <= c[3] && c[3] <= b[3] && b[4] <= c[4] &&
                         c[4] <= c[5] && c[5] <= b[5],
                     CWFA_E_INVAL, "cwfa_footprint_select_f32: core %d [%d,%d) x [%d,%d) x [%d,%d) is not inside its box", i, c[0], c[1], c[2],
                     c[3], c[4], c[5]);
    }
    FP_CHECK(fp_check_offsets("cwfa_footprint_select_f32", boxes, offsets, N));
    CWFA_REQUIRE((corr && w) || offsets[N] == 0, CWFA_E_INVAL, "cwfa_footprint_select_f32: null pointer");
    CWFA_REQUIRE((reinterpret_cast<uintptr_t>(wsum) & 7u) == 0, CWFA_E_ALIGN, "cwfa_footprint_select_f32: wsum must be 8-byte aligned");
    if (N == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int n0 = 0; n0 < N; n0 += FP_CHUNK) {
        const int mm = N - n0 < FP_CHUNK ? N - n0 : FP_CHUNK;
        FpSelect ck;
        const int64_t most = fp_fill_boxes(ck, boxes, n0, mm);
        for (int i = 0; i < FP_CHUNK; ++i) {
            for (int k = 0; k < 6; ++k) ck.core[i][k] = i < mm ? cores[6 * (n0 + i) + k] : 0;
            ck.off[i] = i < mm ? offsets[n0 + i] : 0;
        }
        const unsigned lds = (unsigned)((most + 15) & ~(int64_t)15);   // a byte per voxel of the chunk's largest box, at most 32 KiB
        hipLaunchKernelGGL(footprint_select_kernel, dim3(mm), dim3(FP_SELECT_THREADS), lds, st, corr, ck, thr, w, wsum + n0, size + n0);
        CWFA_LAUNCH_CHECK("cwfa_footprint_select_f32");
    }
    return CWFA_OK;
}
