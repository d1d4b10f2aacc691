// Per-lenslet frame registration with an axial-motion fit: an XLFM frame holds L views of the sample, an axial
// displacement moves view i by a * g_i, and the rigid estimate of section 26 sees none of it.  Four passes around the existing
// whitening, peak and up-sampled-DFT kernels (register_ops.hip), which run unchanged on the [chunk * L, ph, pw] batch of views:
//   rview_*    cuts, widens and tapers the L views of every frame in one read of the stack
//   rlabel_*   the label map of the geometry: which view's box holds a pixel
//   rfit_*     the fit of (d_y, d_x, a) to the L per-view shifts of a frame, float64, one thread per frame, no atomics
//   rshiftl_*  the resampling of register_ops.hip with the shift of every pixel looked up through its label
// The centre table is a HOST array, checked here and handed to the kernels in their arguments (the form of the box tables of
// footprint_ops.hip): what a kernel indexes with is what was checked.  Built with -ffp-contract=off; tests/register_views_ref.py is the
// numpy restatement.
#include <math.h>
#include <type_traits>
#include "common.h"
#include "register_internal.h"

#define RV_MAX_VIEWS 254              // a label is a byte, and label L is "the rest of the frame"

struct RvCenters {
    int c[RV_MAX_VIEWS][2];           // (row, column)
};

// the table's checks, and the kernels' copy of it
static int rv_centers(const char* fn, const int32_t* centers, int L, int ph, int pw, RvCenters& ck) {
    CWFA_REQUIRE(L >= 1 && L <= RV_MAX_VIEWS, CWFA_E_SHAPE, "%s: 1 to %d views are expected, got %d", fn, RV_MAX_VIEWS, L);
    CWFA_REQUIRE(ph >= 1 && pw >= 1, CWFA_E_SHAPE, "%s: a view of %d x %d", fn, ph, pw);
    CWFA_REQUIRE(ph < (1 << 30) && pw < (1 << 30) && (int64_t)ph * pw < ((int64_t)1 << 31), CWFA_E_SHAPE, "%s: a view of %d x %d is too large", fn, ph, pw);
    CWFA_REQUIRE(centers, CWFA_E_INVAL, "%s: null pointer", fn);
    for (int i = 0; i < RV_MAX_VIEWS; ++i) {
        const int cy = i < L ? centers[2 * i] : 0, cx = i < L ? centers[2 * i + 1] : 0;
        // a box start c - size / 2 and a pixel's offset from a centre stay ints, the squared distance an int64
        CWFA_REQUIRE(cy > -(1 << 29) && cy < (1 << 29) && cx > -(1 << 29) && cx < (1 << 29), CWFA_E_INVAL, "%s: centre %d (%d, %d) is out of range", fn, i,
                     cy, cx);
        ck.c[i][0] = cy, ck.c[i][1] = cx;
    }
    return CWFA_OK;
}

#define RV_CHECK(call)          \
    do {                        \
        const int rc_ = (call); \
        if (rc_ != CWFA_OK) return rc_; \
    } while (0)

// ------------------------------------------------------------------------------------------------ the views
// out[n,l,y,x] = fl(float(x[n, cy_l - ph/2 + y, cx_l - pw/2 + x]) * fl(wy[y] * wx[x])), a pixel outside the frame read as 0.0f: the
// cut, the widening and the taper in one read.  A thread owns V pixels of a view's row, keeps their window product and walks the
// frames blockIdx.z, blockIdx.z + gridDim.z, ..; blockIdx.y is the view.  A box starts anywhere: inside the frame the V source pixels
// are one load of element alignment, across its border they are read element by element.
template <int V, bool HALF>
__global__ __launch_bounds__(256) void rview_kernel(const void* __restrict__ x, int N, int H, int W, int64_t fs, const RvCenters ck, int L, int ph,
                                                    int pw, const float* __restrict__ wy, const float* __restrict__ wx, float* __restrict__ out) {
    using elem = std::conditional_t<HALF, _Float16, float>;
    typedef float fvec __attribute__((ext_vector_type(V)));
    const int Wv = pw / V;                                            // V > 1: pw is a multiple of V
    const int q = blockIdx.x * blockDim.x + threadIdx.x;              // ph * pw < 2^31
    if (q >= ph * Wv) return;
    const int vy = q / Wv, vx0 = (q - vy * Wv) * V;
    const int l = blockIdx.y;
    const int y = ck.c[l][0] - ph / 2 + vy, xs = ck.c[l][1] - pw / 2 + vx0;
    float w[V];
    {
        const float a = wy[vy];
#pragma unroll
        for (int j = 0; j < V; ++j) w[j] = __fmul_rn(a, wx[vx0 + j]);
    }
    const bool row_in = y >= 0 && y < H;
    const bool inside = row_in && xs >= 0 && xs <= W - V;
    const int64_t p = (int64_t)(row_in ? y : 0) * W;
    const int64_t o = ((int64_t)l * ph + vy) * pw + vx0, os = (int64_t)L * ph * pw;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        const elem* row = reinterpret_cast<const elem*>(x) + (int64_t)n * fs + p;
        float v[V];
        if (V > 1 && inside) {
            rshift_span<elem, V> sp;
            __builtin_memcpy(&sp, row + xs, sizeof(sp));
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = (float)sp.v[j];
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int xx = xs + j;
                v[j] = row_in && xx >= 0 && xx < W ? (float)row[xx] : 0.f;
            }
        }
        fvec r;
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = __fmul_rn(v[j], w[j]);
        *reinterpret_cast<fvec*>(out + (int64_t)n * os + o) = r;
    }
}

extern "C" int cwfa_reg_window_views(const void* x, int dtype, int N, int H, int W, int64_t frame_stride, const int32_t* centers, int L, int ph,
                                     int pw, const float* wy, const float* wx, float* out, void* stream) {
    const char* fn = "cwfa_reg_window_views";
    CWFA_REQUIRE(x && wy && wx && out && centers, CWFA_E_INVAL, "%s: null pointer", fn);
    CWFA_REQUIRE(dtype == 0 || dtype == 1, CWFA_E_INVAL, "%s: dtype is 0 (fp32) or 1 (fp16), got %d", fn, dtype);
    CWFA_REQUIRE(N >= 0, CWFA_E_SHAPE, "%s: negative size", fn);
    CWFA_REQUIRE(H >= 1 && W >= 1, CWFA_E_SHAPE, "%s: a frame of %d x %d", fn, H, W);
    CWFA_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) && H < (1 << 30) && W < (1 << 30), CWFA_E_SHAPE, "%s: a frame of %d x %d is too large", fn, H, W);
    RvCenters ck;
    RV_CHECK(rv_centers(fn, centers, L, ph, pw, ck));
    CWFA_REQUIRE(frame_stride >= (int64_t)H * W, CWFA_E_INVAL, "%s: frame stride smaller than a frame", fn);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(wy) | reinterpret_cast<uintptr_t>(wx) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0, CWFA_E_ALIGN,
                 "%s: wy, wx and out must be 4-byte aligned", fn);
    CWFA_REQUIRE(static_cast<const void*>(out) != x, CWFA_E_INVAL, "%s: out must not be the stack", fn);
    if (N == 0) return CWFA_OK;
    const bool v4 = (pw & 3) == 0 && cwfa_aligned16(out);             // 16-byte stores: every row of every view then starts on 16 bytes
    const int64_t gx = (((int64_t)ph * pw >> (v4 ? 2 : 0)) + 255) / 256;
    const dim3 grid((unsigned)gx, (unsigned)L, reg_grid_y(gx * L, N, 65536));
    hipStream_t st = (hipStream_t)stream;
#define RVIEW_LAUNCH(V, HALF) \
    hipLaunchKernelGGL((rview_kernel<V, HALF>), grid, dim3(256), 0, st, x, N, H, W, frame_stride, ck, L, ph, pw, wy, wx, out)
    if (v4) { if (dtype) RVIEW_LAUNCH(4, true); else RVIEW_LAUNCH(4, false); }
    else { if (dtype) RVIEW_LAUNCH(1, true); else RVIEW_LAUNCH(1, false); }
#undef RVIEW_LAUNCH
    CWFA_LAUNCH_CHECK("cwfa_reg_window_views");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the label map
// labels[y,x] = the view whose box holds the pixel; among several the one with the smallest integer squared distance to its centre,
// ties to the lowest index; L where no box holds it.  One thread per pixel, the views in order (a uniform loop over the arguments).
__global__ __launch_bounds__(256) void rlabel_kernel(const RvCenters ck, int L, int ph, int pw, int H, int W, unsigned char* __restrict__ labels) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)H * W) return;
    const int y = (int)(q / W), x = (int)(q - (int64_t)y * W);
    int best = L;
    int64_t bd = 0;
    for (int i = 0; i < L; ++i) {
        const int cy = ck.c[i][0], cx = ck.c[i][1];
        const int y0 = cy - ph / 2, x0 = cx - pw / 2;
        if (y < y0 || y - y0 >= ph || x < x0 || x - x0 >= pw) continue;
        const int64_t ey = (int64_t)y - cy, ex = (int64_t)x - cx, d = ey * ey + ex * ex;
        if (best == L || d < bd) best = i, bd = d;
    }
    labels[q] = (unsigned char)best;
}

extern "C" int cwfa_reg_label_map(const int32_t* centers, int L, int ph, int pw, int H, int W, uint8_t* labels, void* stream) {
    const char* fn = "cwfa_reg_label_map";
    CWFA_REQUIRE(centers && labels, CWFA_E_INVAL, "%s: null pointer", fn);
    CWFA_REQUIRE(H >= 1 && W >= 1, CWFA_E_SHAPE, "%s: a frame of %d x %d", fn, H, W);
    CWFA_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) && H < (1 << 30) && W < (1 << 30), CWFA_E_SHAPE, "%s: a frame of %d x %d is too large", fn, H, W);
    RvCenters ck;
    RV_CHECK(rv_centers(fn, centers, L, ph, pw, ck));
    const int64_t P = (int64_t)H * W;
    hipLaunchKernelGGL(rlabel_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ck, L, ph, pw, H, W, labels);
    CWFA_LAUNCH_CHECK("cwfa_reg_label_map");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the fit
// One thread per frame, everything float64, every sum over the views in order i = 0 .. L - 1 from 0.0 (a view of weight 0 is
// skipped), every product, sum, difference and quotient rounded on its own:
//   m = sum w;  gm = (sum w g) / m;  sm = (sum w s) / m;  q = sum w (ey ey + ex ex), e = g - gm;
//   a = q > 0 ? (sum w (ey ty + ex tx)) / q : 0, t = s - sm;  d = sm - a gm.
// The weights live in `inlier` between the passes: the thread that wrote a byte reads it.
struct rfit_result {
    double dy, dx, a;
};

__device__ __forceinline__ bool rfit_once(const float* __restrict__ s, const double* __restrict__ g, const unsigned char* w, int L, rfit_result& f) {
    double m = 0.0, gy = 0.0, gx = 0.0, sy = 0.0, sx = 0.0;
    for (int i = 0; i < L; ++i) {
        if (!w[i]) continue;
        m = m + 1.0;
        gy = gy + g[2 * i], gx = gx + g[2 * i + 1];
        sy = sy + (double)s[2 * i], sx = sx + (double)s[2 * i + 1];
    }
    if (!(m >= 1.0)) return false;
    gy = gy / m, gx = gx / m, sy = sy / m, sx = sx / m;
    double q = 0.0, c = 0.0;
    for (int i = 0; i < L; ++i) {
        if (!w[i]) continue;
        const double ey = g[2 * i] - gy, ex = g[2 * i + 1] - gx;
        const double ty = (double)s[2 * i] - sy, tx = (double)s[2 * i + 1] - sx;
        q = q + (ey * ey + ex * ex);
        c = c + (ey * ty + ex * tx);
    }
    f.a = q > 0.0 ? c / q : 0.0;
    f.dy = sy - f.a * gy, f.dx = sx - f.a * gx;
    return true;
}

__global__ __launch_bounds__(64) void rfit_kernel(const float* __restrict__ shifts, const float* __restrict__ peak, const double* __restrict__ g, int N,
                                                  int L, double min_peak, double reject, int model, double* __restrict__ params,
                                                  unsigned char* inlier, float* __restrict__ table) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* s = shifts + n * L * 2;
    unsigned char* w = inlier + n * L;
    for (int i = 0; i < L; ++i) {
        const double p = (double)peak[n * L + i];
        w[i] = fabs(p) < (double)INFINITY && p >= min_peak ? 1 : 0;
    }
    rfit_result f = {0.0, 0.0, 0.0};
    if (rfit_once(s, g, w, L, f)) {
        int left = 0, gone = 0;
        for (int i = 0; i < L; ++i) {
            if (!w[i]) continue;
            const double ry = fabs((double)s[2 * i] - (f.dy + f.a * g[2 * i])), rx = fabs((double)s[2 * i + 1] - (f.dx + f.a * g[2 * i + 1]));
            if ((ry > rx ? ry : rx) > reject) w[i] = 2, ++gone;         // marked, not yet dropped: the first weights may have to come back
            else ++left;
        }
        if (gone && left) {
            for (int i = 0; i < L; ++i) w[i] = w[i] == 1 ? 1 : 0;
            rfit_once(s, g, w, L, f);
        } else if (gone) {                                            // nothing left: the first fit and the first weights
            for (int i = 0; i < L; ++i) w[i] = w[i] ? 1 : 0;
        }
    }
    params[3 * n] = f.dy, params[3 * n + 1] = f.dx, params[3 * n + 2] = f.a;
    float* t = table + n * (L + 1) * 2;
    for (int i = 0; i < L; ++i) {
        const bool measured = model == 1 && w[i];
        t[2 * i] = measured ? s[2 * i] : (float)(f.dy + f.a * g[2 * i]);
        t[2 * i + 1] = measured ? s[2 * i + 1] : (float)(f.dx + f.a * g[2 * i + 1]);
    }
    t[2 * L] = (float)f.dy, t[2 * L + 1] = (float)f.dx;
}

extern "C" int cwfa_reg_fit_views_f64(const float* shifts, const float* peak, const double* directions, int N, int L, double min_peak, double reject,
                                      int model, double* params, uint8_t* inlier, float* table, void* stream) {
    const char* fn = "cwfa_reg_fit_views_f64";
    CWFA_REQUIRE(shifts && peak && directions && params && inlier && table, CWFA_E_INVAL, "%s: null pointer", fn);
    CWFA_REQUIRE(N >= 0, CWFA_E_SHAPE, "%s: negative size", fn);
    CWFA_REQUIRE(L >= 1 && L <= RV_MAX_VIEWS, CWFA_E_SHAPE, "%s: 1 to %d views are expected, got %d", fn, RV_MAX_VIEWS, L);
    CWFA_REQUIRE(model == 0 || model == 1, CWFA_E_INVAL, "%s: model is 0 (axial) or 1 (free), got %d", fn, model);
    CWFA_REQUIRE(min_peak >= 0.0 && reject >= 0.0, CWFA_E_INVAL, "%s: min_peak and reject are not negative and not NaN", fn);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(directions) | reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(table)) & 7u) == 0 &&
                     ((reinterpret_cast<uintptr_t>(shifts) | reinterpret_cast<uintptr_t>(peak)) & 3u) == 0,
                 CWFA_E_ALIGN, "%s: directions, params and table must be 8-byte aligned, shifts and peak 4-byte aligned", fn);
    if (N == 0) return CWFA_OK;
    hipLaunchKernelGGL(rfit_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, shifts, peak, directions, N, L, min_peak, reject,
                       model, params, inlier, table);
    CWFA_LAUNCH_CHECK("cwfa_reg_fit_views_f64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the labelled resampling
// rshift_kernel with (dy, dx) = table[n, min(labels[y,x], L)].  A thread writes V consecutive pixels of a row and reads their V labels
// once, in front of the frames, into one 64-bit word.  Per frame it resamples the whole group under the label of its first pixel
// not yet done -- the rigid kernel's own code, V + 1 source pixels per row in one load -- and keeps the pixels that carry that label:
// one pass everywhere but on the few columns where a box ends, two there (one per label in the group).  Every pixel comes out of
// rshift_pixels under its own label's shift, and rshift_pixels computes a pixel from its own taps alone: the bits cannot depend on
// how the pixels were grouped.
template <int V, bool HALF>
__global__ __launch_bounds__(256) void rshiftl_kernel(const void* __restrict__ in, int N, int H, int W, int64_t fs, const f32x2* __restrict__ table,
                                                      const unsigned char* __restrict__ labels, int L, int nearest, float fill, void* __restrict__ out) {
    using elem = std::conditional_t<HALF, _Float16, float>;
    typedef elem evec __attribute__((ext_vector_type(V)));
    const int Wv = W / V;                                             // V > 1: W is a multiple of V
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)H * Wv) return;
    const int y = (int)(q / Wv), x0 = (int)(q - (int64_t)y * Wv) * V;
    uint64_t lab = 0;                                                 // byte j: min(label of pixel j, L)
    {
        rshift_span<unsigned char, V> lb;
        __builtin_memcpy(&lb, labels + (int64_t)y * W + x0, sizeof(lb));
#pragma unroll
        for (int j = 0; j < V; ++j) lab |= (uint64_t)(lb.v[j] < L ? lb.v[j] : L) << (8 * j);
    }
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const f32x2* tn = table + (int64_t)n * (L + 1);
        const elem* src = reinterpret_cast<const elem*>(in) + (int64_t)n * fs;
        elem* o = reinterpret_cast<elem*>(out) + (int64_t)n * H * W + (int64_t)y * W + x0;
        float acc[V];
        unsigned todo = (1u << V) - 1u;
        while (todo) {
            const int l = (int)((lab >> (8 * __builtin_ctz(todo))) & 0xFFu);
            const f32x2 s = tn[l];
            float a[V];
            rshift_pixels<V, elem>(src, H, W, y, x0, s[0], s[1], nearest, fill, a);
#pragma unroll
            for (int j = 0; j < V; ++j)
                if ((int)((lab >> (8 * j)) & 0xFFu) == l) acc[j] = a[j], todo &= ~(1u << j);
        }
        evec r;
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = (elem)acc[j];
        *reinterpret_cast<evec*>(o) = r;
    }
}

extern "C" int cwfa_reg_shift_labeled(const void* in, int dtype, int N, int H, int W, int64_t frame_stride, const float* table, const uint8_t* labels,
                                      int L, int mode, float fill, void* out, void* stream) {
    const char* fn = "cwfa_reg_shift_labeled";
    CWFA_REQUIRE(in && table && labels && out, CWFA_E_INVAL, "%s: null pointer", fn);
    CWFA_REQUIRE(dtype == 0 || dtype == 1, CWFA_E_INVAL, "%s: dtype is 0 (fp32) or 1 (fp16), got %d", fn, dtype);
    CWFA_REQUIRE(mode == 0 || mode == 1, CWFA_E_INVAL, "%s: mode is 0 (bilinear) or 1 (nearest), got %d", fn, mode);
    CWFA_REQUIRE(N >= 0, CWFA_E_SHAPE, "%s: negative size", fn);
    CWFA_REQUIRE(L >= 1 && L <= RV_MAX_VIEWS, CWFA_E_SHAPE, "%s: 1 to %d views are expected, got %d", fn, RV_MAX_VIEWS, L);
    CWFA_REQUIRE(H >= 1 && W >= 1, CWFA_E_SHAPE, "%s: a frame of %d x %d", fn, H, W);
    CWFA_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) && H < (1 << 30) && W < (1 << 30), CWFA_E_SHAPE, "%s: a frame of %d x %d is too large", fn, H, W);
    CWFA_REQUIRE(frame_stride >= (int64_t)H * W, CWFA_E_INVAL, "%s: frame stride smaller than a frame", fn);
    CWFA_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7u) == 0, CWFA_E_ALIGN, "%s: table must be 8-byte aligned", fn);
    CWFA_REQUIRE(out != in, CWFA_E_INVAL, "%s: out must not alias the stack", fn);
    if (N == 0) return CWFA_OK;
    const int64_t P = (int64_t)H * W;
    const f32x2* tb = reinterpret_cast<const f32x2*>(table);
    REG_SHIFT_LAUNCH(rshiftl_kernel, reg_store_width(dtype, W, out), dtype, P, N, (hipStream_t)stream, in, N, H, W, frame_stride, tb, labels, L, mode,
                     fill, out);
    CWFA_LAUNCH_CHECK("cwfa_reg_shift_labeled");
    return CWFA_OK;
}
