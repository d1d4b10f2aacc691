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
