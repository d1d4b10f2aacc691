// Richardson-Lucy deconvolution (reference utils.py:465-550, 630-738): everything between the FFTs of XLFMDeconv, fft_conv and
// fft_conv_split.  The FFTs themselves stay with rocFFT (torch.fft).  All HBM-bound streaming kernels: every plane is read and
// written once per kernel, offsets are 64-bit (120 x 2760 x 1381 complex values are more than 4 GB), accesses are 16 bytes wide
// where the shapes and pointers allow and element by element where they do not.  Built with -ffp-contract=off: every fp32 operation
// is rounded separately.
#include <math.h>
#include "common.h"

#define DC_THREADS 256

// ------------------------------------------------------------------------------------------------ spectrum product
// out[z][i] = a[z or 0][i] * (conj ? conj(otf[z][i]) : otf[z][i]) on interleaved complex64 (utils.py:501,700,715).
// One block covers DC_THREADS * 4 units of V complex values of one plane; grid.y walks the planes.  In place (out == a) is safe:
// a thread reads its elements before it writes them.
template <int V>
__global__ __launch_bounds__(DC_THREADS) void spectrum_mul_kernel(const float* a, const float* __restrict__ otf, float* out, int64_t units,
                                                                  int64_t plane, int conj) {
    typedef float vec __attribute__((ext_vector_type(2 * V)));
    const int64_t z = blockIdx.y;
    const vec* pa = reinterpret_cast<const vec*>(a);      // one plane for every z, or the one long plane
    const vec* pb = reinterpret_cast<const vec*>(otf + z * plane);
    vec* po = reinterpret_cast<vec*>(out + z * plane);
    const int64_t base = (int64_t)blockIdx.x * (DC_THREADS * 4) + threadIdx.x;
    vec va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = base + u * DC_THREADS;
        if (i < units) va[u] = pa[i], vb[u] = pb[i];
    }
    const float sg = conj ? -1.0f : 1.0f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = base + u * DC_THREADS;
        if (i >= units) continue;
        vec r;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float ar = va[u][2 * j], ai = va[u][2 * j + 1], br = vb[u][2 * j], bi = sg * vb[u][2 * j + 1];
            r[2 * j] = ar * br - ai * bi;
            r[2 * j + 1] = ar * bi + ai * br;
        }
        po[i] = r;
    }
}

extern "C" int cwfa_deconv_spectrum_mul_c64(const float* a, const float* otf, float* out, int D, int64_t n, int a_planes, int conj,
                                            void* stream) {
    CWFA_REQUIRE(a && otf && out, CWFA_E_INVAL, "cwfa_deconv_spectrum_mul_c64: null pointer");
    CWFA_REQUIRE(D >= 0 && n >= 0 && D <= 65535 && n < ((int64_t)1 << 40), CWFA_E_SHAPE, "cwfa_deconv_spectrum_mul_c64: bad shape (D = %d, n = %lld)",
                 D, (long long)n);
    CWFA_REQUIRE(a_planes == D || a_planes == 1, CWFA_E_INVAL, "cwfa_deconv_spectrum_mul_c64: a holds %d planes, neither 1 nor D = %d", a_planes, D);
    CWFA_REQUIRE(otf != out, CWFA_E_INVAL, "cwfa_deconv_spectrum_mul_c64: the transfer function is never written (out == otf)");
    if (D == 0 || n == 0) return CWFA_OK;
    // a full set of planes is one long plane; a broadcast plane is walked per depth
    const bool bcast = a_planes == 1 && D > 1;
    const int planes = bcast ? D : 1;
    const int64_t len = bcast ? n : n * D;
    const bool vec = cwfa_aligned16(a) && cwfa_aligned16(otf) && cwfa_aligned16(out) && (len & 1) == 0;
    const int64_t units = vec ? len >> 1 : len;
    const int64_t blocks = (units + DC_THREADS * 4 - 1) / (DC_THREADS * 4);
    CWFA_REQUIRE(blocks < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_deconv_spectrum_mul_c64: grid too large");
    const dim3 grid((unsigned)blocks, planes);
    if (vec)
        hipLaunchKernelGGL(spectrum_mul_kernel<2>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, a, otf, out, units, 2 * n, conj);
    else
        hipLaunchKernelGGL(spectrum_mul_kernel<1>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, a, otf, out, units, 2 * n, conj);
    CWFA_LAUNCH_CHECK("cwfa_deconv_spectrum_mul_c64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ shifted depth sum
// out[s][y][x] (+)= post(sum_z pre(p[s][z][(y + oy + sy) mod H][(x + ox + sx) mod W])), sy = ceil(H / 2), sx = ceil(W / 2):
// batch_fftshift2d_real (utils.py:465-477: the source index is the target index plus the shift), the relu and depth sum of
// utils.py:700, the crop, depth sum and abs of utils.py:545-546.  One thread owns V adjacent output pixels and walks z.
template <int V>
__global__ __launch_bounds__(DC_THREADS) void project_kernel(const float* __restrict__ p, float* __restrict__ out, int D, int H, int W, int Ho,
                                                             int Wo, int ys, int xs, int pre, int post, int accumulate) {
    typedef float vec __attribute__((ext_vector_type(V)));
    const int gw = Wo / V;
    const int64_t g = (int64_t)blockIdx.x * DC_THREADS + threadIdx.x;
    if (g >= (int64_t)Ho * gw) return;
    const int y = (int)(g / gw), x = (int)(g % gw) * V;
    int srow = y + ys, scol = x + xs;                 // ys, xs < H, W: one conditional subtraction wraps
    if (srow >= H) srow -= H;
    if (scol >= W) scol -= W;
    const int64_t hw = (int64_t)H * W;
    const float* src = p + (int64_t)blockIdx.y * D * hw + (int64_t)srow * W + scol;
    vec acc;
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    for (int z = 0; z < D; ++z) {
        vec v = *reinterpret_cast<const vec*>(src + z * hw);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += pre ? (v[j] > 0.f ? v[j] : (v[j] != v[j] ? v[j] : 0.f)) : v[j];
    }
    vec* dst = reinterpret_cast<vec*>(out + ((int64_t)blockIdx.y * Ho + y) * Wo + x);
    vec o;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = 0.f;
    if (accumulate) o = *dst;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = accumulate ? o[j] + (post ? fabsf(acc[j]) : acc[j]) : (post ? fabsf(acc[j]) : acc[j]);
    *dst = o;
}

extern "C" int cwfa_deconv_project_f32(const float* p, float* out, int N, int D, int H, int W, int Ho, int Wo, int oy, int ox, int pre,
                                       int post, int accumulate, void* stream) {
    CWFA_REQUIRE(p && out, CWFA_E_INVAL, "cwfa_deconv_project_f32: null pointer");
    CWFA_REQUIRE(N >= 0 && D >= 0 && H >= 0 && W >= 0 && Ho >= 0 && Wo >= 0 && N <= 65535 && (int64_t)H * W < ((int64_t)1 << 31), CWFA_E_SHAPE,
                 "cwfa_deconv_project_f32: bad shape");
    CWFA_REQUIRE(oy >= 0 && ox >= 0 && (int64_t)oy + Ho <= H && (int64_t)ox + Wo <= W, CWFA_E_INVAL,
                 "cwfa_deconv_project_f32: the %d x %d window at (%d, %d) is not inside the %d x %d plane", Ho, Wo, oy, ox, H, W);
    CWFA_REQUIRE(pre == CWFA_DECONV_PRE_NONE || pre == CWFA_DECONV_PRE_RELU, CWFA_E_INVAL, "cwfa_deconv_project_f32: unknown pre %d", pre);
    CWFA_REQUIRE(post == CWFA_DECONV_POST_NONE || post == CWFA_DECONV_POST_ABS, CWFA_E_INVAL, "cwfa_deconv_project_f32: unknown post %d", post);
    if (N == 0 || Ho == 0 || Wo == 0) return CWFA_OK;
    const int ys = (oy + (H + 1) / 2) % H, xs = (ox + (W + 1) / 2) % W;
    // 16-byte groups: no group straddles the wrap column and every source / target address is aligned
    const bool vec = (W & 3) == 0 && (Wo & 3) == 0 && (xs & 3) == 0 && cwfa_aligned16(p) && cwfa_aligned16(out);
    const int64_t groups = (int64_t)Ho * (vec ? Wo / 4 : Wo);
    const dim3 grid((unsigned)((groups + DC_THREADS - 1) / DC_THREADS), N);
    if (vec)
        hipLaunchKernelGGL(project_kernel<4>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, p, out, D, H, W, Ho, Wo, ys, xs, pre, post, accumulate);
    else
        hipLaunchKernelGGL(project_kernel<1>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, p, out, D, H, W, Ho, Wo, ys, xs, pre, post, accumulate);
    CWFA_LAUNCH_CHECK("cwfa_deconv_project_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ ratio image
// tmp = img / (est + 1e-8f) (utils.py:701).  *flag |= 1 where tmp is NaN or img is not finite: the reference starts from
// ImgEst = 0 * ImgExp (utils.py:677), so a non-finite pixel is NaN in every estimate and stops its loop (utils.py:707).
template <int V>
__global__ __launch_bounds__(DC_THREADS) void ratio_kernel(const float* __restrict__ img, const float* __restrict__ est, float* __restrict__ tmp,
                                                           int* __restrict__ flag, int64_t units) {
    typedef float vec __attribute__((ext_vector_type(V)));
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * DC_THREADS + threadIdx.x; i < units; i += (int64_t)gridDim.x * DC_THREADS) {
        const vec a = reinterpret_cast<const vec*>(img)[i], e = reinterpret_cast<const vec*>(est)[i];
        vec r;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            r[j] = a[j] / (e[j] + 1e-8f);
            bad |= (r[j] != r[j]) || !isfinite(a[j]);
        }
        reinterpret_cast<vec*>(tmp)[i] = r;
    }
    if (bad) atomicOr(flag, 1);
}

static inline unsigned deconv_blocks(int64_t units) {
    const int64_t b = (units + DC_THREADS - 1) / DC_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

extern "C" int cwfa_deconv_ratio_f32(const float* img, const float* est, float* tmp, int* flag, int64_t n, void* stream) {
    CWFA_REQUIRE(img && est && tmp && flag, CWFA_E_INVAL, "cwfa_deconv_ratio_f32: null pointer");
    CWFA_REQUIRE(n >= 0, CWFA_E_SHAPE, "cwfa_deconv_ratio_f32: negative size");
    if (n == 0) return CWFA_OK;
    if ((n & 3) == 0 && cwfa_aligned16(img) && cwfa_aligned16(est) && cwfa_aligned16(tmp))
        hipLaunchKernelGGL(ratio_kernel<4>, dim3(deconv_blocks(n >> 2)), dim3(DC_THREADS), 0, (hipStream_t)stream, img, est, tmp, flag, n >> 2);
    else
        hipLaunchKernelGGL(ratio_kernel<1>, dim3(deconv_blocks(n)), dim3(DC_THREADS), 0, (hipStream_t)stream, img, est, tmp, flag, n);
    CWFA_LAUNCH_CHECK("cwfa_deconv_ratio_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ clamp at a device bound
// In place torch.clamp_(tmp, 0, *median * mult) (utils.py:702-703): min(max(x, 0), hi), NaN kept; nothing when *count == 0.
template <int V>
__global__ __launch_bounds__(DC_THREADS) void clamp_kernel(float* __restrict__ tmp, int64_t units, const float* __restrict__ median,
                                                           const long long* __restrict__ count, float mult) {
    typedef float vec __attribute__((ext_vector_type(V)));
    if (*count == 0) return;
    const float hi = *median * mult;
    for (int64_t i = (int64_t)blockIdx.x * DC_THREADS + threadIdx.x; i < units; i += (int64_t)gridDim.x * DC_THREADS) {
        vec v = reinterpret_cast<vec*>(tmp)[i];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float x = v[j];
            x = x < 0.f ? 0.f : x;
            x = x > hi ? hi : x;
            v[j] = x;
        }
        reinterpret_cast<vec*>(tmp)[i] = v;
    }
}

extern "C" int cwfa_deconv_clamp_f32(float* tmp, int64_t n, const float* median, const int64_t* count, float mult, void* stream) {
    CWFA_REQUIRE(tmp && median && count, CWFA_E_INVAL, "cwfa_deconv_clamp_f32: null pointer");
    CWFA_REQUIRE(n >= 0, CWFA_E_SHAPE, "cwfa_deconv_clamp_f32: negative size");
    if (n == 0) return CWFA_OK;
    const long long* cnt = reinterpret_cast<const long long*>(count);
    if ((n & 3) == 0 && cwfa_aligned16(tmp))
        hipLaunchKernelGGL(clamp_kernel<4>, dim3(deconv_blocks(n >> 2)), dim3(DC_THREADS), 0, (hipStream_t)stream, tmp, n >> 2, median, cnt, mult);
    else
        hipLaunchKernelGGL(clamp_kernel<1>, dim3(deconv_blocks(n)), dim3(DC_THREADS), 0, (hipStream_t)stream, tmp, n, median, cnt, mult);
    CWFA_LAUNCH_CHECK("cwfa_deconv_clamp_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ object update
// obj_pad[z][po + y][po + x] *= b[z][(po + y + s) mod F][(po + x + s) mod F], s = ceil(F / 2), over the interior obj x obj window
// (utils.py:715: the product with the shifted back projection, then the negative pad).  The object stays zero-padded between the
// iterations: only the window of either tensor is touched, the border of obj_pad stays exactly 0.
template <int V>
__global__ __launch_bounds__(DC_THREADS) void update_kernel(float* __restrict__ obj_pad, const float* __restrict__ b, int F, int obj, int po,
                                                            int shift) {
    typedef float vec __attribute__((ext_vector_type(V)));
    const int gw = obj / V;
    const int64_t g = (int64_t)blockIdx.x * DC_THREADS + threadIdx.x;
    if (g >= (int64_t)obj * gw) return;
    const int y = po + (int)(g / gw), x = po + (int)(g % gw) * V;
    int srow = y + shift, scol = x + shift;
    if (srow >= F) srow -= F;
    if (scol >= F) scol -= F;
    const int64_t plane = (int64_t)blockIdx.y * F * F;
    vec* dst = reinterpret_cast<vec*>(obj_pad + plane + (int64_t)y * F + x);
    const vec m = *reinterpret_cast<const vec*>(b + plane + (int64_t)srow * F + scol);
    vec v = *dst;
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = v[j] * m[j];
    *dst = v;
}

extern "C" int cwfa_deconv_update_f32(float* obj_pad, const float* b, int D, int F, int obj, int po, void* stream) {
    CWFA_REQUIRE(obj_pad && b, CWFA_E_INVAL, "cwfa_deconv_update_f32: null pointer");
    CWFA_REQUIRE(D >= 0 && F >= 0 && obj >= 0 && D <= 65535 && (int64_t)F * F < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_deconv_update_f32: bad shape");
    CWFA_REQUIRE(po >= 0 && (int64_t)po + obj <= F, CWFA_E_INVAL, "cwfa_deconv_update_f32: the %d x %d window at %d is not inside the %d x %d plane",
                 obj, obj, po, F, F);
    CWFA_REQUIRE(obj_pad != b, CWFA_E_INVAL, "cwfa_deconv_update_f32: the object and the back projection are the same tensor");
    if (D == 0 || obj == 0) return CWFA_OK;
    const int shift = (F + 1) / 2;
    const bool vec = (F & 3) == 0 && (obj & 3) == 0 && (po & 3) == 0 && (shift & 3) == 0 && cwfa_aligned16(obj_pad) && cwfa_aligned16(b);
    const int64_t groups = (int64_t)obj * (vec ? obj / 4 : obj);
    const dim3 grid((unsigned)((groups + DC_THREADS - 1) / DC_THREADS), D);
    if (vec)
        hipLaunchKernelGGL(update_kernel<4>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, obj_pad, b, F, obj, po, shift);
    else
        hipLaunchKernelGGL(update_kernel<1>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, obj_pad, b, F, obj, po, shift);
    CWFA_LAUNCH_CHECK("cwfa_deconv_update_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ vector extrapolation
// Biggs-Andrews acceleration of the iteration above.  The padded object holds the prediction y_k; the iterates
// x_k, x_{k+1} and the step g live in window-sized buffers [D][obj][obj].  A block owns DC_THREADS * 4 units of V window elements of
// one depth (CWFA_DECONV_ACCEL_UNITS); the window has fewer than 2^31 elements per depth, so its indices are 32-bit.
#define DC_ALPHA_THREADS 1024

// x_new = y * shifted(b) (the one fp32 product of update_kernel), g = x_new - y; slab row (depth in chunk, block) += the float64
// partials of sum g * g_prev and sum g_prev^2.  The chunks of one iteration run one after the other on the stream, so a row receives
// its chunks' partials in chunk order; no atomics.  g == g_prev is safe: a thread reads its elements before it writes them.
template <int V>
__global__ __launch_bounds__(DC_THREADS) void update_accel_kernel(const float* __restrict__ obj_pad, const float* __restrict__ b, const float* g_prev,
                                                                  float* __restrict__ x_new, float* g, double* __restrict__ slab, int F, int obj,
                                                                  int po, int shift) {
    typedef float vec __attribute__((ext_vector_type(V)));
    __shared__ double red[16];
    const unsigned gw = obj / V, units = (unsigned)obj * gw;
    const unsigned base = blockIdx.x * (DC_THREADS * 4) + threadIdx.x;
    const int64_t plane = (int64_t)blockIdx.y * F * F, win = (int64_t)blockIdx.y * obj * obj;
    vec vy[4], vm[4], vp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned i = base + u * DC_THREADS;
        if (i >= units) continue;
        const int y = po + (int)(i / gw), x = po + (int)(i % gw) * V;
        int srow = y + shift, scol = x + shift;
        if (srow >= F) srow -= F;
        if (scol >= F) scol -= F;
        vy[u] = *reinterpret_cast<const vec*>(obj_pad + plane + (int64_t)y * F + x);
        vm[u] = *reinterpret_cast<const vec*>(b + plane + (int64_t)srow * F + scol);
        vp[u] = *reinterpret_cast<const vec*>(g_prev + win + (int64_t)i * V);
    }
    double dot = 0.0, nrm = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned i = base + u * DC_THREADS;
        if (i >= units) continue;
        vec xn, gn;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            xn[j] = vy[u][j] * vm[u][j];
            gn[j] = xn[j] - vy[u][j];
            dot += (double)gn[j] * (double)vp[u][j];               // fp32 x fp32 is exact in float64
            nrm += (double)vp[u][j] * (double)vp[u][j];
        }
        *reinterpret_cast<vec*>(x_new + win + (int64_t)i * V) = xn;
        *reinterpret_cast<vec*>(g + win + (int64_t)i * V) = gn;
    }
    dot = cwfa_block_sum(dot, red);
    nrm = cwfa_block_sum(nrm, red);
    if (threadIdx.x == 0) {
        const int64_t row = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        slab[2 * row] += dot;
        slab[2 * row + 1] += nrm;
    }
}

// the window in 16-byte groups: every row of either tensor starts on a 16-byte boundary and no group straddles the wrap column
static inline bool accel_vec(int F, int obj, int po) { return (F & 3) == 0 && (obj & 3) == 0 && (po & 3) == 0; }

static inline int64_t accel_blocks(int obj, bool vec) {
    const int64_t units = (int64_t)obj * (vec ? obj / 4 : obj);
    return (units + CWFA_DECONV_ACCEL_UNITS - 1) / CWFA_DECONV_ACCEL_UNITS;
}

extern "C" int cwfa_deconv_update_accel_f32(const float* obj_pad, const float* b, const float* g_prev, float* x_new, float* g, double* slab,
                                            int64_t slab_rows, int D, int F, int obj, int po, void* stream) {
    CWFA_REQUIRE(obj_pad && b && g_prev && x_new && g && slab, CWFA_E_INVAL, "cwfa_deconv_update_accel_f32: null pointer");
    CWFA_REQUIRE(D >= 0 && F >= 0 && obj >= 0 && D <= 65535 && (int64_t)F * F < ((int64_t)1 << 31), CWFA_E_SHAPE,
                 "cwfa_deconv_update_accel_f32: bad shape");
    CWFA_REQUIRE(po >= 0 && (int64_t)po + obj <= F, CWFA_E_INVAL,
                 "cwfa_deconv_update_accel_f32: the %d x %d window at %d is not inside the %d x %d plane", obj, obj, po, F, F);
    CWFA_REQUIRE(obj_pad != b, CWFA_E_INVAL, "cwfa_deconv_update_accel_f32: the object and the back projection are the same tensor");
    CWFA_REQUIRE(x_new != g && x_new != g_prev && (const float*)x_new != obj_pad && (const float*)x_new != b && (const float*)g != obj_pad &&
                     (const float*)g != b,
                 CWFA_E_INVAL, "cwfa_deconv_update_accel_f32: x_new and g are written: they share no buffer with an input or each other");
    CWFA_REQUIRE((reinterpret_cast<uintptr_t>(slab) & 7u) == 0, CWFA_E_ALIGN, "cwfa_deconv_update_accel_f32: the slab is not 8-byte aligned");
    if (D == 0 || obj == 0) return CWFA_OK;
    const int shift = (F + 1) / 2;
    const bool vec = accel_vec(F, obj, po) && (shift & 3) == 0 && cwfa_aligned16(obj_pad) && cwfa_aligned16(b) && cwfa_aligned16(g_prev) &&
                     cwfa_aligned16(x_new) && cwfa_aligned16(g);
    const int64_t blocks = accel_blocks(obj, vec);
    CWFA_REQUIRE(slab_rows >= blocks * D, CWFA_E_INVAL, "cwfa_deconv_update_accel_f32: the slab holds %lld rows, %d depths need %lld",
                 (long long)slab_rows, D, (long long)(blocks * D));
    const dim3 grid((unsigned)blocks, D);
    if (vec)
        hipLaunchKernelGGL(update_accel_kernel<4>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, obj_pad, b, g_prev, x_new, g, slab, F, obj, po,
                           shift);
    else
        hipLaunchKernelGGL(update_accel_kernel<1>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, obj_pad, b, g_prev, x_new, g, slab, F, obj, po,
                           shift);
    CWFA_LAUNCH_CHECK("cwfa_deconv_update_accel_f32");
    return CWFA_OK;
}

// *alpha = clamp(sum of column 0 / sum of column 1, 0, alpha_max), 0 when the quotient is not finite (an empty or zero denominator
// included); each thread adds its rows in ascending order, then the block sum: one fixed order.  The slab is left zeroed.
__global__ __launch_bounds__(DC_ALPHA_THREADS) void alpha_kernel(double* __restrict__ slab, int64_t rows, double alpha_max,
                                                                 float* __restrict__ alpha) {
    __shared__ double red[16];
    double num = 0.0, den = 0.0;
    for (int64_t i = threadIdx.x; i < rows; i += DC_ALPHA_THREADS) {
        num += slab[2 * i];
        den += slab[2 * i + 1];
        slab[2 * i] = 0.0;
        slab[2 * i + 1] = 0.0;
    }
    num = cwfa_block_sum(num, red);
    den = cwfa_block_sum(den, red);
    if (threadIdx.x == 0) {
        const double q = num / den;
        *alpha = (float)(isfinite(q) ? (q < 0.0 ? 0.0 : (q > alpha_max ? alpha_max : q)) : 0.0);
    }
}

extern "C" int cwfa_deconv_alpha_f64(double* slab, int64_t rows, double alpha_max, float* alpha, void* stream) {
    CWFA_REQUIRE(slab && alpha, CWFA_E_INVAL, "cwfa_deconv_alpha_f64: null pointer");
    CWFA_REQUIRE(rows >= 0, CWFA_E_SHAPE, "cwfa_deconv_alpha_f64: negative size");
    CWFA_REQUIRE(alpha_max >= 0.0 && alpha_max < 1.0, CWFA_E_INVAL, "cwfa_deconv_alpha_f64: alpha_max = %g is not in [0, 1)", alpha_max);
    CWFA_REQUIRE((reinterpret_cast<uintptr_t>(slab) & 7u) == 0 && (reinterpret_cast<uintptr_t>(alpha) & 3u) == 0, CWFA_E_ALIGN,
                 "cwfa_deconv_alpha_f64: the slab is not 8-byte or alpha not 4-byte aligned");
    hipLaunchKernelGGL(alpha_kernel, dim3(1), dim3(DC_ALPHA_THREADS), 0, (hipStream_t)stream, slab, rows, alpha_max, alpha);
    CWFA_LAUNCH_CHECK("cwfa_deconv_alpha_f64");
    return CWFA_OK;
}

// obj_pad window = max(x_new + *alpha * (x_new - x_prev), 0): difference, product and sum are rounded one by one; NaN is kept.
template <int V>
__global__ __launch_bounds__(DC_THREADS) void predict_kernel(float* __restrict__ obj_pad, const float* __restrict__ x_new,
                                                             const float* __restrict__ x_prev, const float* __restrict__ alpha, int F, int obj,
                                                             int po) {
    typedef float vec __attribute__((ext_vector_type(V)));
    const float a = *alpha;
    const unsigned gw = obj / V, units = (unsigned)obj * gw;
    const unsigned base = blockIdx.x * (DC_THREADS * 4) + threadIdx.x;
    const int64_t plane = (int64_t)blockIdx.y * F * F, win = (int64_t)blockIdx.y * obj * obj;
    vec vn[4], vo[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned i = base + u * DC_THREADS;
        if (i >= units) continue;
        vn[u] = *reinterpret_cast<const vec*>(x_new + win + (int64_t)i * V);
        vo[u] = *reinterpret_cast<const vec*>(x_prev + win + (int64_t)i * V);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned i = base + u * DC_THREADS;
        if (i >= units) continue;
        vec r;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = vn[u][j] - vo[u][j];
            const float t = a * d;
            const float s = vn[u][j] + t;
            r[j] = s > 0.f ? s : (s != s ? s : 0.f);
        }
        const int y = po + (int)(i / gw), x = po + (int)(i % gw) * V;
        *reinterpret_cast<vec*>(obj_pad + plane + (int64_t)y * F + x) = r;
    }
}

extern "C" int cwfa_deconv_predict_f32(float* obj_pad, const float* x_new, const float* x_prev, const float* alpha, int D, int F, int obj, int po,
                                       void* stream) {
    CWFA_REQUIRE(obj_pad && x_new && x_prev && alpha, CWFA_E_INVAL, "cwfa_deconv_predict_f32: null pointer");
    CWFA_REQUIRE(D >= 0 && F >= 0 && obj >= 0 && D <= 65535 && (int64_t)F * F < ((int64_t)1 << 31), CWFA_E_SHAPE,
                 "cwfa_deconv_predict_f32: bad shape");
    CWFA_REQUIRE(po >= 0 && (int64_t)po + obj <= F, CWFA_E_INVAL, "cwfa_deconv_predict_f32: the %d x %d window at %d is not inside the %d x %d plane",
                 obj, obj, po, F, F);
    CWFA_REQUIRE((const float*)obj_pad != x_new && (const float*)obj_pad != x_prev, CWFA_E_INVAL,
                 "cwfa_deconv_predict_f32: the padded object and an iterate are the same tensor");
    if (D == 0 || obj == 0) return CWFA_OK;
    const bool vec = accel_vec(F, obj, po) && cwfa_aligned16(obj_pad) && cwfa_aligned16(x_new) && cwfa_aligned16(x_prev);
    const dim3 grid((unsigned)accel_blocks(obj, vec), D);
    if (vec)
        hipLaunchKernelGGL(predict_kernel<4>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, obj_pad, x_new, x_prev, alpha, F, obj, po);
    else
        hipLaunchKernelGGL(predict_kernel<1>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, obj_pad, x_new, x_prev, alpha, F, obj, po);
    CWFA_LAUNCH_CHECK("cwfa_deconv_predict_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ MAP update under a Gaussian prior
// The EM M-step of a Poisson likelihood with an independent prior N(mu, 1 / w) per voxel: the x > 0 that
// maximises -x + a log x - w / 2 (x - mu)^2, a the plain Richardson-Lucy update, i.e. the positive root of w x^2 + c x - a = 0,
// c = 1 - w mu, in the form that only adds terms of one sign.  Nine fp32 operations, each rounded once.  Square root and division are
// sqrtf and /, which hipcc expands to the correctly rounded sequences by default (-fhip-fp32-correctly-rounded-divide-sqrt); the
// __fsqrt_rn intrinsic is the native approximation in this toolchain and is not used.  The tests compare bits with IEEE arithmetic.
// w == 0 gives c = 1, r = 1 and 2a / 2 = a: the plain update's bits.  The test is c > 0, not >=: c == 0 with a == 0 would be 0 / 0
// in the first form.  a < 0 (a back projection's rounding noise below zero) can make the discriminant negative; it is held at 0
// there, which changes nothing for a >= 0.  NaN is kept.
__device__ __forceinline__ float map_step(float a, float mu, float w) {
    const float wm = w * mu;
    const float c = 1.0f - wm;
    const float wa = w * a;
    const float cc = c * c;
    const float t = cc + 4.0f * wa;                                  // the product with 4 is exact
    const float r = sqrtf(t < 0.f ? 0.f : t);
    return c > 0.f ? (2.0f * a) / (c + r) : (r - c) / (2.0f * w);
}

// the prior's penalty of one input element, 0.5 w (y - mu)^2, every operation in float64
__device__ __forceinline__ double map_penalty(float y, float mu, float w) {
    const double d = (double)y - (double)mu;
    return 0.5 * (double)w * (d * d);
}

// update_kernel's walk: the window of obj_pad becomes M(window * shifted(b), mu, w); mu and w are window-sized [D][obj][obj].
// With a penalty slab, row (depth in chunk, block) += the block's float64 sum of the penalty of the window as it was read.
static_assert(CWFA_DECONV_UPDATE_UNITS == DC_THREADS, "one unit per thread");

template <int V>
__global__ __launch_bounds__(DC_THREADS) void update_map_kernel(float* __restrict__ obj_pad, const float* __restrict__ b,
                                                                const float* __restrict__ mu, const float* __restrict__ w,
                                                                double* __restrict__ pen, int F, int obj, int po, int shift) {
    typedef float vec __attribute__((ext_vector_type(V)));
    __shared__ double red[16];
    const int gw = obj / V;
    const int64_t g = (int64_t)blockIdx.x * DC_THREADS + threadIdx.x;
    double acc = 0.0;
    if (g < (int64_t)obj * gw) {
        const int y = po + (int)(g / gw), x = po + (int)(g % gw) * V;
        int srow = y + shift, scol = x + shift;
        if (srow >= F) srow -= F;
        if (scol >= F) scol -= F;
        const int64_t plane = (int64_t)blockIdx.y * F * F, win = (int64_t)blockIdx.y * obj * obj + g * V;
        vec* dst = reinterpret_cast<vec*>(obj_pad + plane + (int64_t)y * F + x);
        const vec m = *reinterpret_cast<const vec*>(b + plane + (int64_t)srow * F + scol);
        const vec vm = *reinterpret_cast<const vec*>(mu + win), vw = *reinterpret_cast<const vec*>(w + win);
        vec v = *dst;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            acc += map_penalty(v[j], vm[j], vw[j]);
            v[j] = map_step(v[j] * m[j], vm[j], vw[j]);
        }
        *dst = v;
    }
    if (pen == nullptr) return;                                      // uniform over the block
    acc = cwfa_block_sum(acc, red);
    if (threadIdx.x == 0) pen[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] += acc;
}

extern "C" int cwfa_deconv_update_map_f32(float* obj_pad, const float* b, const float* mu, const float* w, double* pen_slab, int64_t pen_rows,
                                          int D, int F, int obj, int po, void* stream) {
    CWFA_REQUIRE(obj_pad && b && mu && w, CWFA_E_INVAL, "cwfa_deconv_update_map_f32: null pointer");
    CWFA_REQUIRE(D >= 0 && F >= 0 && obj >= 0 && D <= 65535 && (int64_t)F * F < ((int64_t)1 << 31), CWFA_E_SHAPE,
                 "cwfa_deconv_update_map_f32: bad shape");
    CWFA_REQUIRE(po >= 0 && (int64_t)po + obj <= F, CWFA_E_INVAL, "cwfa_deconv_update_map_f32: the %d x %d window at %d is not inside the %d x %d plane",
                 obj, obj, po, F, F);
    CWFA_REQUIRE(obj_pad != b, CWFA_E_INVAL, "cwfa_deconv_update_map_f32: the object and the back projection are the same tensor");
    CWFA_REQUIRE((const float*)obj_pad != mu && (const float*)obj_pad != w, CWFA_E_INVAL,
                 "cwfa_deconv_update_map_f32: the object is written: it shares no buffer with the prior");
    CWFA_REQUIRE((reinterpret_cast<uintptr_t>(pen_slab) & 7u) == 0, CWFA_E_ALIGN, "cwfa_deconv_update_map_f32: the penalty slab is not 8-byte aligned");
    if (D == 0 || obj == 0) return CWFA_OK;
    const int shift = (F + 1) / 2;
    const bool vec = accel_vec(F, obj, po) && (shift & 3) == 0 && cwfa_aligned16(obj_pad) && cwfa_aligned16(b) && cwfa_aligned16(mu) &&
                     cwfa_aligned16(w);
    const int64_t groups = (int64_t)obj * (vec ? obj / 4 : obj);
    const int64_t blocks = (groups + DC_THREADS - 1) / DC_THREADS;
    CWFA_REQUIRE(pen_slab == nullptr || pen_rows >= blocks * D, CWFA_E_INVAL,
                 "cwfa_deconv_update_map_f32: the penalty slab holds %lld rows, %d depths need %lld", (long long)pen_rows, D, (long long)(blocks * D));
    const dim3 grid((unsigned)blocks, D);
    if (vec)
        hipLaunchKernelGGL(update_map_kernel<4>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, obj_pad, b, mu, w, pen_slab, F, obj, po, shift);
    else
        hipLaunchKernelGGL(update_map_kernel<1>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, obj_pad, b, mu, w, pen_slab, F, obj, po, shift);
    CWFA_LAUNCH_CHECK("cwfa_deconv_update_map_f32");
    return CWFA_OK;
}

// update_accel_kernel's walk: x_new = M(y * shifted(b), mu, w), g = x_new - y, the same two float64 slab columns for alpha_kernel;
// with a penalty slab, row (depth in chunk, block) += the block's float64 sum of the penalty of y.
template <int V>
__global__ __launch_bounds__(DC_THREADS) void update_accel_map_kernel(const float* __restrict__ obj_pad, const float* __restrict__ b,
                                                                      const float* g_prev, const float* __restrict__ mu,
                                                                      const float* __restrict__ w, float* __restrict__ x_new, float* g,
                                                                      double* __restrict__ slab, double* __restrict__ pen, int F, int obj, int po,
                                                                      int shift) {
    typedef float vec __attribute__((ext_vector_type(V)));
    __shared__ double red[16];
    const unsigned gw = obj / V, units = (unsigned)obj * gw;
    const unsigned base = blockIdx.x * (DC_THREADS * 4) + threadIdx.x;
    const int64_t plane = (int64_t)blockIdx.y * F * F, win = (int64_t)blockIdx.y * obj * obj;
    vec vy[4], vm[4], vp[4], vmu[4], vw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned i = base + u * DC_THREADS;
        if (i >= units) continue;
        const int y = po + (int)(i / gw), x = po + (int)(i % gw) * V;
        int srow = y + shift, scol = x + shift;
        if (srow >= F) srow -= F;
        if (scol >= F) scol -= F;
        vy[u] = *reinterpret_cast<const vec*>(obj_pad + plane + (int64_t)y * F + x);
        vm[u] = *reinterpret_cast<const vec*>(b + plane + (int64_t)srow * F + scol);
        vp[u] = *reinterpret_cast<const vec*>(g_prev + win + (int64_t)i * V);
        vmu[u] = *reinterpret_cast<const vec*>(mu + win + (int64_t)i * V);
        vw[u] = *reinterpret_cast<const vec*>(w + win + (int64_t)i * V);
    }
    double dot = 0.0, nrm = 0.0, acc = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned i = base + u * DC_THREADS;
        if (i >= units) continue;
        vec xn, gn;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            xn[j] = map_step(vy[u][j] * vm[u][j], vmu[u][j], vw[u][j]);
            gn[j] = xn[j] - vy[u][j];
            dot += (double)gn[j] * (double)vp[u][j];
            nrm += (double)vp[u][j] * (double)vp[u][j];
            acc += map_penalty(vy[u][j], vmu[u][j], vw[u][j]);
        }
        *reinterpret_cast<vec*>(x_new + win + (int64_t)i * V) = xn;
        *reinterpret_cast<vec*>(g + win + (int64_t)i * V) = gn;
    }
    dot = cwfa_block_sum(dot, red);
    nrm = cwfa_block_sum(nrm, red);
    if (pen != nullptr) acc = cwfa_block_sum(acc, red);
    if (threadIdx.x == 0) {
        const int64_t row = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        slab[2 * row] += dot;
        slab[2 * row + 1] += nrm;
        if (pen != nullptr) pen[row] += acc;
    }
}

extern "C" int cwfa_deconv_update_accel_map_f32(const float* obj_pad, const float* b, const float* g_prev, const float* mu, const float* w,
                                                float* x_new, float* g, double* slab, int64_t slab_rows, double* pen_slab, int64_t pen_rows, int D,
                                                int F, int obj, int po, void* stream) {
    CWFA_REQUIRE(obj_pad && b && g_prev && mu && w && x_new && g && slab, CWFA_E_INVAL, "cwfa_deconv_update_accel_map_f32: null pointer");
    CWFA_REQUIRE(D >= 0 && F >= 0 && obj >= 0 && D <= 65535 && (int64_t)F * F < ((int64_t)1 << 31), CWFA_E_SHAPE,
                 "cwfa_deconv_update_accel_map_f32: bad shape");
    CWFA_REQUIRE(po >= 0 && (int64_t)po + obj <= F, CWFA_E_INVAL,
                 "cwfa_deconv_update_accel_map_f32: the %d x %d window at %d is not inside the %d x %d plane", obj, obj, po, F, F);
    CWFA_REQUIRE(obj_pad != b, CWFA_E_INVAL, "cwfa_deconv_update_accel_map_f32: the object and the back projection are the same tensor");
    CWFA_REQUIRE(x_new != g && x_new != g_prev && (const float*)x_new != obj_pad && (const float*)x_new != b && (const float*)x_new != mu &&
                     (const float*)x_new != w && (const float*)g != obj_pad && (const float*)g != b && (const float*)g != mu &&
                     (const float*)g != w,
                 CWFA_E_INVAL, "cwfa_deconv_update_accel_map_f32: x_new and g are written: they share no buffer with an input or each other");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(slab) | reinterpret_cast<uintptr_t>(pen_slab)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_deconv_update_accel_map_f32: a slab is not 8-byte aligned");
    CWFA_REQUIRE(slab != pen_slab, CWFA_E_INVAL, "cwfa_deconv_update_accel_map_f32: the two slabs are the same buffer");
    if (D == 0 || obj == 0) return CWFA_OK;
    const int shift = (F + 1) / 2;
    const bool vec = accel_vec(F, obj, po) && (shift & 3) == 0 && cwfa_aligned16(obj_pad) && cwfa_aligned16(b) && cwfa_aligned16(g_prev) &&
                     cwfa_aligned16(mu) && cwfa_aligned16(w) && cwfa_aligned16(x_new) && cwfa_aligned16(g);
    const int64_t blocks = accel_blocks(obj, vec);
    CWFA_REQUIRE(slab_rows >= blocks * D, CWFA_E_INVAL, "cwfa_deconv_update_accel_map_f32: the slab holds %lld rows, %d depths need %lld",
                 (long long)slab_rows, D, (long long)(blocks * D));
    CWFA_REQUIRE(pen_slab == nullptr || pen_rows >= blocks * D, CWFA_E_INVAL,
                 "cwfa_deconv_update_accel_map_f32: the penalty slab holds %lld rows, %d depths need %lld", (long long)pen_rows, D,
                 (long long)(blocks * D));
    const dim3 grid((unsigned)blocks, D);
    if (vec)
        hipLaunchKernelGGL(update_accel_map_kernel<4>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, obj_pad, b, g_prev, mu, w, x_new, g, slab,
                           pen_slab, F, obj, po, shift);
    else
        hipLaunchKernelGGL(update_accel_map_kernel<1>, grid, dim3(DC_THREADS), 0, (hipStream_t)stream, obj_pad, b, g_prev, mu, w, x_new, g, slab,
                           pen_slab, F, obj, po, shift);
    CWFA_LAUNCH_CHECK("cwfa_deconv_update_accel_map_f32");
    return CWFA_OK;
}

// trace[index] += the sum of the penalty slab's rows: each thread adds its rows in ascending order, then the block sum, one fixed
// order, onto the likelihood cwfa_deconv_poisson_nll_f32 wrote there.  The slab is left zeroed.
__global__ __launch_bounds__(DC_ALPHA_THREADS) void penalty_kernel(double* __restrict__ slab, int64_t rows, double* __restrict__ out) {
    __shared__ double red[16];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < rows; i += DC_ALPHA_THREADS) {
        acc += slab[i];
        slab[i] = 0.0;
    }
    acc = cwfa_block_sum(acc, red);
    if (threadIdx.x == 0) *out += acc;
}

extern "C" int cwfa_deconv_penalty_f64(double* slab, int64_t rows, double* trace, int64_t index, int64_t trace_len, void* stream) {
    CWFA_REQUIRE(slab && trace, CWFA_E_INVAL, "cwfa_deconv_penalty_f64: null pointer");
    CWFA_REQUIRE(rows >= 0, CWFA_E_SHAPE, "cwfa_deconv_penalty_f64: negative size");
    CWFA_REQUIRE(index >= 0 && index < trace_len, CWFA_E_INVAL, "cwfa_deconv_penalty_f64: element %lld is not inside a trace of %lld",
                 (long long)index, (long long)trace_len);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(slab) | reinterpret_cast<uintptr_t>(trace)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_deconv_penalty_f64: the slab or the trace is not 8-byte aligned");
    CWFA_REQUIRE(slab != trace, CWFA_E_INVAL, "cwfa_deconv_penalty_f64: the slab and the trace are the same buffer");
    if (rows == 0) return CWFA_OK;
    hipLaunchKernelGGL(penalty_kernel, dim3(1), dim3(DC_ALPHA_THREADS), 0, (hipStream_t)stream, slab, rows, trace + index);
    CWFA_LAUNCH_CHECK("cwfa_deconv_penalty_f64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ Poisson likelihood
// sum over the image of est - img * log(est + 1e-8), every term and every sum in float64: per-block partials, then one block adds
// them in ascending order and writes one element of the trace.
#define DC_NLL_BLOCKS (CWFA_DECONV_NLL_WORKSPACE_BYTES / 8)

template <int V>
__global__ __launch_bounds__(DC_THREADS) void nll_kernel(const float* __restrict__ img, const float* __restrict__ est, double* __restrict__ partial,
                                                         int64_t units) {
    typedef float vec __attribute__((ext_vector_type(V)));
    __shared__ double red[16];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * DC_THREADS + threadIdx.x; i < units; i += (int64_t)gridDim.x * DC_THREADS) {
        const vec a = reinterpret_cast<const vec*>(img)[i], e = reinterpret_cast<const vec*>(est)[i];
#pragma unroll
        for (int j = 0; j < V; ++j) acc += (double)e[j] - (double)a[j] * log((double)e[j] + 1e-8);
    }
    acc = cwfa_block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(DC_THREADS) void nll_finish_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
    __shared__ double red[16];
    double acc = 0.0;
    for (int i = threadIdx.x; i < blocks; i += DC_THREADS) acc += partial[i];
    acc = cwfa_block_sum(acc, red);
    if (threadIdx.x == 0) *out = acc;
}

extern "C" int cwfa_deconv_poisson_nll_f32(const float* img, const float* est, int64_t n, double* trace, int64_t index, int64_t trace_len,
                                           void* workspace, void* stream) {
    CWFA_REQUIRE(img && est && trace && workspace, CWFA_E_INVAL, "cwfa_deconv_poisson_nll_f32: null pointer");
    CWFA_REQUIRE(n >= 0, CWFA_E_SHAPE, "cwfa_deconv_poisson_nll_f32: negative size");
    CWFA_REQUIRE(index >= 0 && index < trace_len, CWFA_E_INVAL, "cwfa_deconv_poisson_nll_f32: element %lld is not inside a trace of %lld",
                 (long long)index, (long long)trace_len);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(trace) | reinterpret_cast<uintptr_t>(workspace)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_deconv_poisson_nll_f32: the trace or the workspace is not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(trace + index, 0, sizeof(double), st) != hipSuccess) {
            cwfa_set_error("cwfa_deconv_poisson_nll_f32: clearing the element failed");
            return CWFA_E_HIP;
        }
        return CWFA_OK;
    }
    double* partial = static_cast<double*>(workspace);
    const bool vec = (n & 3) == 0 && cwfa_aligned16(img) && cwfa_aligned16(est);
    const int64_t units = vec ? n >> 2 : n;
    const unsigned want = deconv_blocks(units), blocks = want > DC_NLL_BLOCKS ? DC_NLL_BLOCKS : want;
    if (vec)
        hipLaunchKernelGGL(nll_kernel<4>, dim3(blocks), dim3(DC_THREADS), 0, st, img, est, partial, units);
    else
        hipLaunchKernelGGL(nll_kernel<1>, dim3(blocks), dim3(DC_THREADS), 0, st, img, est, partial, units);
    CWFA_LAUNCH_CHECK("cwfa_deconv_poisson_nll_f32");
    hipLaunchKernelGGL(nll_finish_kernel, dim3(1), dim3(DC_THREADS), 0, st, partial, (int)blocks, trace + index);
    CWFA_LAUNCH_CHECK("cwfa_deconv_poisson_nll_f32");
    return CWFA_OK;
}
