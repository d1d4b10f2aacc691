// Rigid frame registration in front of sparse-activity extraction: phase correlation of every frame of a stack
// against a template, an integer peak in a bounded window with parabolic sub-pixel refinement, and resampling.  rocFFT (through
// torch.fft) does the transforms; the four passes around them are here: the edge taper (the kernel of register_internal.h, which
// the volumes of section 30 share), the whitened cross-power (rwht_*), the peak (rpeak_*) and the resampling (rshift_*).
// The shifts stay on the device from the peak kernel to the resampling kernel.  Behind them the up-sampled DFT that refines the
// peak from the whitened spectra (rups_*, rfp_*; section 26.5).  Built with -ffp-contract=off; the products, sums and differences
// the restatement (tests/register_ref.py) counts are spelled with the __f*_rn intrinsics all the same, the square root and the
// divisions with sqrtf and / (see rwht_one).
#include <math.h>
#include <type_traits>
#include "common.h"
#include "register_internal.h"

// ------------------------------------------------------------------------------------------------ the window
// out[n,y,x] = fl(float(x[n,y,x]) * fl(wy[y] * wx[x])): reg_window_kernel (register_internal.h) over [N, 1, H, W] without a z factor.
extern "C" int cwfa_reg_window(const void* x, int dtype, int N, int H, int W, int64_t frame_stride, const float* wy, const float* wx,
                               float* out, void* stream) {
    CWFA_REQUIRE(x && wy && wx && out, CWFA_E_INVAL, "cwfa_reg_window: null pointer");
    CWFA_REQUIRE(dtype == 0 || dtype == 1, CWFA_E_INVAL, "cwfa_reg_window: dtype is 0 (fp32) or 1 (fp16), got %d", dtype);
    CWFA_REQUIRE(N >= 0 && H >= 0 && W >= 0, CWFA_E_SHAPE, "cwfa_reg_window: negative size");
    CWFA_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_reg_window: a frame of %d x %d is too large", H, W);
    if (N == 0 || H == 0 || W == 0) return CWFA_OK;
    const int64_t P = (int64_t)H * W;
    CWFA_REQUIRE(frame_stride >= P, CWFA_E_INVAL, "cwfa_reg_window: frame stride smaller than a frame");
    CWFA_REQUIRE(static_cast<const void*>(out) != x, CWFA_E_INVAL, "cwfa_reg_window: out must not be the stack");
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x);
    const bool v4 = (W & 3) == 0 && (frame_stride & 3) == 0 && cwfa_aligned16(wx) && cwfa_aligned16(out) && (xa & (dtype ? 7u : 15u)) == 0;
    reg_window_launch(x, dtype == 1, N, 1, H, W, frame_stride, nullptr, wy, wx, out, v4, (hipStream_t)stream);
    CWFA_LAUNCH_CHECK("cwfa_reg_window");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the whitened cross-power
// u = z / (|z| + eps), |z| = sqrtf(fl(fl(re re) + fl(im im))), and with a weight plane out = u * w (four products, one difference,
// one sum, all rounded).  A thread owns a bin, keeps its weight and walks the frames, so the plane is read once per launch (per
// block row); a bin is 8 bytes, a wave reads 512 consecutive bytes per frame, four frames in flight.  out may be F: an element is
// read before it is written, by the same thread.
template <bool WEIGHT>
__device__ __forceinline__ f32x2 rwht_one(f32x2 z, f32x2 w, float eps) {
    // sqrtf and / are the correctly rounded forms (hipcc's default); __fsqrt_rn is the native approximation in this tool chain
    const float m = sqrtf(__fadd_rn(__fmul_rn(z[0], z[0]), __fmul_rn(z[1], z[1])));
    const float d = __fadd_rn(m, eps);
    const float ur = z[0] / d, ui = z[1] / d;
    if constexpr (!WEIGHT) return f32x2{ur, ui};
    return f32x2{__fsub_rn(__fmul_rn(ur, w[0]), __fmul_rn(ui, w[1])), __fadd_rn(__fmul_rn(ur, w[1]), __fmul_rn(ui, w[0]))};
}

template <bool WEIGHT>
__global__ __launch_bounds__(256) void rwht_kernel(const f32x2* F, const f32x2* __restrict__ Wt, int N, int64_t bins, float eps, f32x2* out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= bins) return;
    f32x2 w = f32x2{0.f, 0.f};
    if constexpr (WEIGHT) w = Wt[k];
    const int step = gridDim.y;
    int n = blockIdx.y;
    for (; n + 3 * step < N; n += 4 * step) {
        f32x2 z[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = F[(int64_t)(n + j * step) * bins + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) out[(int64_t)(n + j * step) * bins + k] = rwht_one<WEIGHT>(z[j], w, eps);
    }
    for (; n < N; n += step) out[(int64_t)n * bins + k] = rwht_one<WEIGHT>(F[(int64_t)n * bins + k], w, eps);
}

extern "C" int cwfa_reg_whiten_c64(const void* F, const void* Wt, int N, int64_t bins, float eps, void* out, void* stream) {
    CWFA_REQUIRE(F && out, CWFA_E_INVAL, "cwfa_reg_whiten_c64: null pointer");
    CWFA_REQUIRE(eps >= 0.f && eps < INFINITY, CWFA_E_INVAL, "cwfa_reg_whiten_c64: eps must be finite and not negative");
    CWFA_REQUIRE(N >= 0 && bins >= 0, CWFA_E_SHAPE, "cwfa_reg_whiten_c64: negative size");
    CWFA_REQUIRE((bins + 255) / 256 < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_reg_whiten_c64: too many bins");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(F) | reinterpret_cast<uintptr_t>(Wt) | reinterpret_cast<uintptr_t>(out)) & 7u) == 0, CWFA_E_ALIGN,
                 "cwfa_reg_whiten_c64: complex64 data must be 8-byte aligned");
    CWFA_REQUIRE(Wt == nullptr || (Wt != F && Wt != out), CWFA_E_INVAL, "cwfa_reg_whiten_c64: the weight plane must not be F or out");
    if (N == 0 || bins == 0) return CWFA_OK;
    const int64_t gx = (bins + 255) / 256;
    const dim3 grid((unsigned)gx, reg_grid_y(gx, N, 8192));
    hipStream_t st = (hipStream_t)stream;
    const f32x2* f = static_cast<const f32x2*>(F);
    const f32x2* w = static_cast<const f32x2*>(Wt);
    f32x2* o = static_cast<f32x2*>(out);
    if (Wt) hipLaunchKernelGGL((rwht_kernel<true>), grid, dim3(256), 0, st, f, w, N, bins, eps, o);
    else hipLaunchKernelGGL((rwht_kernel<false>), grid, dim3(256), 0, st, f, w, N, bins, eps, o);
    CWFA_LAUNCH_CHECK("cwfa_reg_whiten_c64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the peak
// One workgroup per frame.  Window index i (row-major from (-my, -mx)) reads c at (sy mod H, sx mod W); the key is reg_peak_key
// (register_internal.h): NaN below everything, ties to the lowest index.  The maximum over a thread's indices, over the wave by
// shuffles, over the waves through the LDS: no atomics, and no trace of the order the threads ran in.  Thread 0 then reads the
// peak's four neighbours (modulo H / W: they may lie outside the window) and fits the two parabolas in float64.
__global__ __launch_bounds__(REG_PEAK_THREADS) void rpeak_kernel(const float* __restrict__ c, int H, int W, int64_t fs, int my, int mx, int subpixel,
                                                                 float* __restrict__ shifts, int* __restrict__ ipeak, float* __restrict__ peak) {
    __shared__ rkey_t best[REG_PEAK_THREADS / 64];
    __shared__ int finite[REG_PEAK_THREADS / 64];
    const int n = blockIdx.x;
    const float* cn = c + (int64_t)n * fs;
    const int wh = 2 * my + 1, ww = 2 * mx + 1;
    const unsigned nwin = (unsigned)wh * (unsigned)ww;                // <= H * W < 2^31
    rkey_t k = 0;
    bool fin = false;
    for (unsigned i = threadIdx.x; i < nwin; i += REG_PEAK_THREADS) {
        const int r = (int)(i / (unsigned)ww), sy = r - my, sx = (int)(i - (unsigned)r * (unsigned)ww) - mx;
        const int y = sy < 0 ? sy + H : sy, x = sx < 0 ? sx + W : sx;   // |sy| < H and |sx| < W: the window fits the frame
        const float v = cn[(int64_t)y * W + x];
        const rkey_t kv = reg_peak_key(v, i);
        k = kv > k ? kv : k;
        fin = fin || fabsf(v) < INFINITY;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const rkey_t other = __shfl_xor(k, o, 64);
        k = other > k ? other : k;
    }
    const bool wave_fin = __ballot(fin) != 0;
    if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = k, finite[threadIdx.x >> 6] = wave_fin ? 1 : 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int any = 0;
#pragma unroll
    for (int w = 0; w < REG_PEAK_THREADS / 64; ++w) {
        k = best[w] > k ? best[w] : k;
        any |= finite[w];
    }
    if (!any) {                                                       // no finite value in the window
        shifts[2 * n] = 0.f, shifts[2 * n + 1] = 0.f;
        ipeak[2 * n] = 0, ipeak[2 * n + 1] = 0;
        peak[n] = __builtin_nanf("");
        return;
    }
    const unsigned i = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
    const int r = (int)(i / (unsigned)ww), sy = r - my, sx = (int)(i - (unsigned)r * (unsigned)ww) - mx;
    const int y = sy < 0 ? sy + H : sy, x = sx < 0 ? sx + W : sx;
    const float c0 = cn[(int64_t)y * W + x];
    double dy = 0.0, dx = 0.0;
    if (subpixel) {
        const int ym = y == 0 ? H - 1 : y - 1, yp = y + 1 == H ? 0 : y + 1;
        const int xm = x == 0 ? W - 1 : x - 1, xp = x + 1 == W ? 0 : x + 1;
        dy = reg_parabola((double)cn[(int64_t)ym * W + x], (double)c0, (double)cn[(int64_t)yp * W + x]);
        dx = reg_parabola((double)cn[(int64_t)y * W + xm], (double)c0, (double)cn[(int64_t)y * W + xp]);
    }
    shifts[2 * n] = (float)((double)sy + dy), shifts[2 * n + 1] = (float)((double)sx + dx);
    ipeak[2 * n] = sy, ipeak[2 * n + 1] = sx;
    peak[n] = c0;
}

extern "C" int cwfa_reg_peak_f32(const float* c, int N, int H, int W, int64_t frame_stride, int my, int mx, int subpixel, float* shifts,
                                 int* ipeak, float* peak, void* stream) {
    CWFA_REQUIRE(c && shifts && ipeak && peak, CWFA_E_INVAL, "cwfa_reg_peak_f32: null pointer");
    CWFA_REQUIRE(subpixel == 0 || subpixel == 1, CWFA_E_INVAL, "cwfa_reg_peak_f32: subpixel is 0 or 1");
    CWFA_REQUIRE(N >= 0 && H >= 0 && W >= 0 && my >= 0 && mx >= 0, CWFA_E_SHAPE, "cwfa_reg_peak_f32: negative size");
    CWFA_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), CWFA_E_SHAPE, "cwfa_reg_peak_f32: a frame of %d x %d is too large", H, W);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(shifts) | reinterpret_cast<uintptr_t>(ipeak)) & 7u) == 0 && (reinterpret_cast<uintptr_t>(peak) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(c) & 3u) == 0,
                 CWFA_E_ALIGN, "cwfa_reg_peak_f32: shifts and ipeak must be 8-byte aligned, c and peak 4-byte aligned");
    if (N == 0 || H == 0 || W == 0) return CWFA_OK;
    CWFA_REQUIRE(2 * (int64_t)my + 1 <= H && 2 * (int64_t)mx + 1 <= W, CWFA_E_SHAPE,
                 "cwfa_reg_peak_f32: the search window (%lld x %lld) is wider than the %d x %d frame", 2 * (long long)my + 1, 2 * (long long)mx + 1, H, W);
    CWFA_REQUIRE(frame_stride >= (int64_t)H * W, CWFA_E_INVAL, "cwfa_reg_peak_f32: frame stride smaller than a frame");
    hipLaunchKernelGGL(rpeak_kernel, dim3((unsigned)N), dim3(REG_PEAK_THREADS), 0, (hipStream_t)stream, c, H, W, frame_stride, my, mx, subpixel,
                       shifts, ipeak, peak);
    CWFA_LAUNCH_CHECK("cwfa_reg_peak_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the resampling
// out[n,y,x] = sum over the taps (0,0), (0,1), (1,0), (1,1) of w * in[n, y + iy + r, x + ix + c], iy = floorf(dy), fy = dy - iy,
// w = fl(wy_r * wx_c) with wy = (fl(1 - fy), fy): every weight and product rounded, the terms added in that order, a tap of
// weight exactly 0 neither read nor added (an integer shift copies bits), a tap outside the frame reads `fill`, a non-finite shift
// fills the frame.  The shift of frame n is read from device memory.  A thread writes V consecutive pixels of a row (a 16-byte
// store: 4 of fp32, 8 of fp16) from the V + 1 source pixels of either row.  The source rows start anywhere: inside the frame the
// span is one load of element alignment (the compiler makes it a vector load plus one element), at the borders element by element.
// The arithmetic is rshift_pixels (register_internal.h), which the labelled resampling of section 29 shares.
template <int V, bool HALF>
__global__ __launch_bounds__(256) void rshift_kernel(const void* __restrict__ in, int N, int H, int W, int64_t fs, const f32x2* __restrict__ shifts,
                                                     int nearest, float fill, void* __restrict__ out) {
    using elem = std::conditional_t<HALF, _Float16, float>;
    typedef elem evec __attribute__((ext_vector_type(V)));
    const int Wv = W / V;                                             // V > 1: W is a multiple of V
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)H * Wv) return;
    const int y = (int)(q / Wv), x0 = (int)(q - (int64_t)y * Wv) * V;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const f32x2 s = shifts[n];
        elem* o = reinterpret_cast<elem*>(out) + (int64_t)n * H * W + (int64_t)y * W + x0;
        float acc[V];
        rshift_pixels<V, elem>(reinterpret_cast<const elem*>(in) + (int64_t)n * fs, H, W, y, x0, s[0], s[1], nearest, fill, acc);
        evec r;
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = (elem)acc[j];
        *reinterpret_cast<evec*>(o) = r;
    }
}

extern "C" int cwfa_reg_shift(const void* in, int dtype, int N, int H, int W, int64_t frame_stride, const float* shifts, int mode, float fill,
                              void* out, void* stream) {
    CWFA_REQUIRE(in && shifts && out, CWFA_E_INVAL, "cwfa_reg_shift: null pointer");
    CWFA_REQUIRE(dtype == 0 || dtype == 1, CWFA_E_INVAL, "cwfa_reg_shift: dtype is 0 (fp32) or 1 (fp16), got %d", dtype);
    CWFA_REQUIRE(mode == 0 || mode == 1, CWFA_E_INVAL, "cwfa_reg_shift: mode is 0 (bilinear) or 1 (nearest), got %d", mode);
    CWFA_REQUIRE(N >= 0 && H >= 0 && W >= 0, CWFA_E_SHAPE, "cwfa_reg_shift: negative size");
    CWFA_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) && H < (1 << 30) && W < (1 << 30), CWFA_E_SHAPE,
                 "cwfa_reg_shift: a frame of %d x %d is too large", H, W);      // y + iy + 1 with |iy| <= H + 1 stays an int
    CWFA_REQUIRE((reinterpret_cast<uintptr_t>(shifts) & 7u) == 0, CWFA_E_ALIGN, "cwfa_reg_shift: shifts must be 8-byte aligned");
    CWFA_REQUIRE(out != in, CWFA_E_INVAL, "cwfa_reg_shift: out must not alias the stack");
    if (N == 0 || H == 0 || W == 0) return CWFA_OK;
    const int64_t P = (int64_t)H * W;
    CWFA_REQUIRE(frame_stride >= P, CWFA_E_INVAL, "cwfa_reg_shift: frame stride smaller than a frame");
    const f32x2* sh = reinterpret_cast<const f32x2*>(shifts);
    REG_SHIFT_LAUNCH(rshift_kernel, reg_store_width(dtype, W, out), dtype, P, N, (hipStream_t)stream, in, N, H, W, frame_stride, sh, mode, fill, out);
    CWFA_LAUNCH_CHECK("cwfa_reg_shift");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the up-sampled DFT (section 26.5)
// The trigonometric interpolant of the correlation on the fine grid y = py + j / u, x = px + j / u, j = -r .. r (U = 2 r + 1), from
// the whitened cross-power R that irfft2 also reads.  Three kernels, all float64, every product and sum rounded on its own:
//   rups_twiddle  Tx[n, kx, j] = w[kx] root_x[(kx m_j) mod (W u)],  Ty[n, ky, j] = root_y[(s(ky) m_j) mod (H u)], m_j = p u + j - r
//                 reduced in integers; the Nyquist column / row keep the real part only; w = 1, 2, .., 2, (1) is exact
//   rups_rows     E[n, ky, j] = sum over kx = 0 .. K - 1, in that order, of R[n, ky, kx] * Tx[n, kx, j]            (the hot pass)
//   rups_cols     C[n, jy, jx] = (sum over ky of Re(Ty[n, ky, jy] * E[n, ky, jx])) * (1 / (H W)), the ky axis in RUPS_SEG segments of
//                 ceil(H / RUPS_SEG) rows, each summed in order from 0.0, the segments then added in order
// The root tables are the caller's (ops.reg_roots): root[k] = exp(2 pi i k / M), k = 0 .. M - 1, interleaved doubles.
// rups_rows: a workgroup owns G * RUPS_RT rows of one frame and a tile of fine columns; a thread owns one fine column and RUPS_RT
// rows: RUPS_RT complex accumulators in registers, one 16-byte twiddle load (coalesced along j) and RUPS_RT broadcast LDS reads per
// kx.  The rows are staged through the LDS RUPS_KC bins at a time, widened to float64 once, read from memory once, coalesced.
#define RUPS_RT 8
#define RUPS_KC 32
#define RUPS_GMAX 8
#define RUPS_SEG 8
#define RUPS_JT 32
typedef double f64x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void rups_twiddle_kernel(const int* __restrict__ ipeak, int H, int W, int u, int r, const f64x2* __restrict__ rootx,
                                                           const f64x2* __restrict__ rooty, f64x2* __restrict__ Tx, f64x2* __restrict__ Ty) {
    const int K = W / 2 + 1, U = 2 * r + 1;
    const int n = blockIdx.y;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nx = (int64_t)K * U, ny = (int64_t)H * U;
    if (q >= nx + ny) return;
    const bool isx = q < nx;
    const int64_t e = isx ? q : q - nx;
    const int k = (int)(e / U), j = (int)(e - (int64_t)k * U);
    const int64_t M = (int64_t)(isx ? W : H) * u;                     // < 2^31
    int64_t m = ((int64_t)ipeak[2 * n + (isx ? 1 : 0)] * u + (j - r)) % M;
    m = m < 0 ? m + M : m;
    const int size = isx ? W : H;
    const int64_t s = isx || 2 * (int64_t)k < H ? k : (int64_t)k - H;
    int64_t idx = (s * m) % M;                                        // |s| < 2^31, m < 2^31
    idx = idx < 0 ? idx + M : idx;
    f64x2 t = (isx ? rootx : rooty)[idx];
    const bool nyq = (size & 1) == 0 && k == size / 2;
    if (nyq) t[1] = 0.0;
    if (isx && k != 0 && !nyq) t = f64x2{2.0 * t[0], 2.0 * t[1]};
    if (isx) Tx[(int64_t)n * nx + e] = t;
    else Ty[(int64_t)n * ny + e] = t;
}

__global__ __launch_bounds__(256) void rups_rows_kernel(const f32x2* __restrict__ R, int H, int K, int64_t fs, int U, int UT, int G,
                                                        const f64x2* __restrict__ Tx, f64x2* __restrict__ E) {
    __shared__ f64x2 z[RUPS_GMAX * RUPS_RT * RUPS_KC];                // 32 KiB
    const int n = blockIdx.z;
    const int rows = G * RUPS_RT;
    const int row0 = blockIdx.x * rows;
    const int g = threadIdx.x / UT, jl = threadIdx.x - g * UT;
    const int j = blockIdx.y * UT + jl;
    const bool active = g < G && j < U;
    const f32x2* Rn = R + (int64_t)n * fs;
    const f64x2* Tn = Tx + (int64_t)n * K * U;
    double ar[RUPS_RT], ai[RUPS_RT];
#pragma unroll
    for (int i = 0; i < RUPS_RT; ++i) ar[i] = 0.0, ai[i] = 0.0;
    // both streams run one step ahead in registers: the next tile of R while this one is summed, the next four twiddles while these
    // four are used (a wave has few neighbours to hide a load behind: the grid is a few workgroups per CU)
    const int sk = threadIdx.x & (RUPS_KC - 1), sr = threadIdx.x / RUPS_KC;
    constexpr int SN = RUPS_GMAX * RUPS_RT * RUPS_KC / 256;
    f32x2 stage[SN];
    auto stage_load = [&](int k0) {
#pragma unroll
        for (int s = 0; s < SN; ++s) {
            const int rr = sr + s * (256 / RUPS_KC), y = row0 + rr, k = k0 + sk;
            stage[s] = rr < rows && y < H && k < K ? Rn[(int64_t)y * K + k] : f32x2{0.f, 0.f};
        }
    };
    auto twiddle = [&](int k) { return Tn[(int64_t)(k < K ? k : K - 1) * U + j]; };     // past the end: the last row again, not used
    stage_load(0);
    f64x2 tn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) tn[q] = active ? twiddle(q) : f64x2{0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += RUPS_KC) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SN; ++s) {
            const int rr = sr + s * (256 / RUPS_KC);
            if (rr < rows) z[rr * RUPS_KC + sk] = f64x2{(double)stage[s][0], (double)stage[s][1]};
        }
        __syncthreads();
        if (k0 + RUPS_KC < K) stage_load(k0 + RUPS_KC);
        if (active) {
            const int kn = K - k0 < RUPS_KC ? K - k0 : RUPS_KC;
            const f64x2* zr = z + g * RUPS_RT * RUPS_KC;
            for (int kk = 0; kk < kn; kk += 4) {                      // RUPS_KC is a multiple of 4: the groups run on across tiles
                f64x2 t[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) t[q] = tn[q];
#pragma unroll
                for (int q = 0; q < 4; ++q) tn[q] = twiddle(k0 + kk + 4 + q);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (kk + q >= kn) break;
#pragma unroll
                    for (int i = 0; i < RUPS_RT; ++i) {
                        const f64x2 v = zr[i * RUPS_KC + kk + q];
                        ar[i] = ar[i] + (v[0] * t[q][0] - v[1] * t[q][1]);
                        ai[i] = ai[i] + (v[0] * t[q][1] + v[1] * t[q][0]);
                    }
                }
            }
        }
    }
    if (!active) return;
    f64x2* En = E + (int64_t)n * H * U;
#pragma unroll
    for (int i = 0; i < RUPS_RT; ++i) {
        const int y = row0 + g * RUPS_RT + i;
        if (y < H) En[(int64_t)y * U + j] = f64x2{ar[i], ai[i]};
    }
}

__global__ __launch_bounds__(RUPS_JT* RUPS_SEG) void rups_cols_kernel(const f64x2* __restrict__ E, const f64x2* __restrict__ Ty, int H, int U, double inv,
                                                                       double* __restrict__ C) {
    __shared__ double part[RUPS_SEG][RUPS_JT];
    const int n = blockIdx.z, jy = blockIdx.y;
    const int jl = threadIdx.x & (RUPS_JT - 1), s = threadIdx.x / RUPS_JT;
    const int jx = blockIdx.x * RUPS_JT + jl;
    const int L = (H + RUPS_SEG - 1) / RUPS_SEG;
    const int y0 = s * L < H ? s * L : H, y1 = H - y0 < L ? H : y0 + L;   // H < 2^30
    const f64x2* En = E + (int64_t)n * H * U;
    const f64x2* Tn = Ty + (int64_t)n * H * U;
    double a = 0.0;
    if (jx < U)
#pragma unroll 4
        for (int y = y0; y < y1; ++y) {
            const f64x2 t = Tn[(int64_t)y * U + jy], v = En[(int64_t)y * U + jx];
            a = a + (t[0] * v[0] - t[1] * v[1]);
        }
    part[s][jl] = a;
    __syncthreads();
    if (s != 0 || jx >= U) return;
    double c = 0.0;
#pragma unroll
    for (int i = 0; i < RUPS_SEG; ++i) c = c + part[i][jl];
    C[((int64_t)n * U + jy) * U + jx] = c * inv;
}

// "reg_upsample_stages" option (measurement only: with a bit cleared the map is not computed): bit 0 launches the twiddle kernel, bit 1
// the row kernel, bit 2 the column kernel
int g_cwfa_reg_upsample_stages = 7;

// the fine grid must stay an int index space and the tables' indices ints
static inline bool rups_sizes_ok(int H, int W, int u, int r) {
    return H >= 1 && W >= 1 && u >= 1 && r >= 1 && H < (1 << 30) && W < (1 << 30) && (int64_t)H * W < ((int64_t)1 << 31) &&
           (int64_t)H * u < ((int64_t)1 << 31) && (int64_t)W * u < ((int64_t)1 << 31) && r < (1 << 14);        // U * U < 2^31
}

extern "C" int64_t cwfa_reg_upsample_workspace_bytes(int N, int H, int W, int r) {
    if (N < 0 || !rups_sizes_ok(H, W, 1, r)) return -1;
    const int64_t U = 2 * (int64_t)r + 1, K = W / 2 + 1;
    return (int64_t)N * (K * U + 2 * (int64_t)H * U) * 16;            // Tx, Ty, E
}

extern "C" int cwfa_reg_upsample_c64(const void* R, int N, int H, int W, int64_t frame_stride, const int* ipeak, int u, int r, const double* rootx,
                                     const double* rooty, double* C, void* ws, void* stream) {
    CWFA_REQUIRE(R && ipeak && rootx && rooty && C && ws, CWFA_E_INVAL, "cwfa_reg_upsample_c64: null pointer");
    CWFA_REQUIRE(N >= 0, CWFA_E_SHAPE, "cwfa_reg_upsample_c64: negative size");
    CWFA_REQUIRE(H >= 1 && W >= 1, CWFA_E_SHAPE, "cwfa_reg_upsample_c64: a frame of %d x %d", H, W);
    CWFA_REQUIRE(u >= 1 && r >= 1, CWFA_E_INVAL, "cwfa_reg_upsample_c64: the factor and the radius are at least 1, got %d and %d", u, r);
    CWFA_REQUIRE(rups_sizes_ok(H, W, u, r), CWFA_E_SHAPE, "cwfa_reg_upsample_c64: %d x %d at factor %d, radius %d is too large", H, W, u, r);
    const int K = W / 2 + 1, U = 2 * r + 1;
    CWFA_REQUIRE(frame_stride >= (int64_t)H * K, CWFA_E_INVAL, "cwfa_reg_upsample_c64: frame stride smaller than a frame's spectrum");
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(ipeak) | reinterpret_cast<uintptr_t>(C)) & 7u) == 0 &&
                     ((reinterpret_cast<uintptr_t>(rootx) | reinterpret_cast<uintptr_t>(rooty) | reinterpret_cast<uintptr_t>(ws)) & 15u) == 0,
                 CWFA_E_ALIGN, "cwfa_reg_upsample_c64: R, ipeak and C must be 8-byte aligned, the root tables and the workspace 16-byte aligned");
    if (N == 0) return CWFA_OK;
    hipStream_t st = (hipStream_t)stream;
    const f64x2 *rx = reinterpret_cast<const f64x2*>(rootx), *ry = reinterpret_cast<const f64x2*>(rooty);
    const int UT = U < 256 ? U : 256, G = 256 / UT < RUPS_GMAX ? 256 / UT : RUPS_GMAX;
    const double inv = 1.0 / (double)((int64_t)H * W);
    const int64_t per = ((int64_t)K + H) * U;
    for (int n0 = 0; n0 < N; n0 += 65535) {                           // a grid axis holds 65535 frames
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        f64x2* Tx = static_cast<f64x2*>(ws) + (int64_t)n0 * K * U;     // the three arrays in turn, each [N, ..]
        f64x2* Ty = static_cast<f64x2*>(ws) + (int64_t)N * K * U + (int64_t)n0 * H * U;
        f64x2* E = static_cast<f64x2*>(ws) + (int64_t)N * ((int64_t)K + H) * U + (int64_t)n0 * H * U;
        const f32x2* Rb = static_cast<const f32x2*>(R) + (int64_t)n0 * frame_stride;
        if (g_cwfa_reg_upsample_stages & 1)
            hipLaunchKernelGGL(rups_twiddle_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)nb), dim3(256), 0, st, ipeak + 2 * (int64_t)n0, H, W, u, r,
                               rx, ry, Tx, Ty);
        if (g_cwfa_reg_upsample_stages & 2)
            hipLaunchKernelGGL(rups_rows_kernel, dim3((unsigned)((H + G * RUPS_RT - 1) / (G * RUPS_RT)), (unsigned)((U + UT - 1) / UT), (unsigned)nb), dim3(256),
                               0, st, Rb, H, K, frame_stride, U, UT, G, Tx, E);
        if (g_cwfa_reg_upsample_stages & 4)
            hipLaunchKernelGGL(rups_cols_kernel, dim3((unsigned)((U + RUPS_JT - 1) / RUPS_JT), (unsigned)U, (unsigned)nb), dim3(RUPS_JT * RUPS_SEG), 0, st, E,
                           Ty, H, U, inv, C + (int64_t)n0 * U * U);
    }
    CWFA_LAUNCH_CHECK("cwfa_reg_upsample_c64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the fine peak
// One workgroup per frame over the fine map C [U, U] (float64): the maximum under the order of the integer peak widened to 64 bits
// (the unsigned image of the bits of c + 0.0, NaN 0, ties to the lowest row-major index), reduced like rpeak_kernel; thread 0 fits
// the float64 parabola per axis where the maximum is not on the grid's border along it.
struct rfp_best {
    uint64_t o;
    unsigned i;
};
__device__ __forceinline__ uint64_t rfp_ord(double v) {
    uint64_t b = __builtin_bit_cast(uint64_t, v);
    b = b == 0x8000000000000000ull ? 0ull : b;
    return v != v ? 0ull : ((b >> 63) ? ~b : (b | 0x8000000000000000ull));
}
__device__ __forceinline__ rfp_best rfp_max(rfp_best a, rfp_best b) { return (b.o > a.o || (b.o == a.o && b.i < a.i)) ? b : a; }

__global__ __launch_bounds__(REG_PEAK_THREADS) void rfp_kernel(const double* __restrict__ C, const int* __restrict__ ipeak, int U, int u, int keep,
                                                               float* __restrict__ shifts, float* __restrict__ peak) {
    __shared__ uint64_t bo[REG_PEAK_THREADS / 64];
    __shared__ unsigned bi[REG_PEAK_THREADS / 64];
    __shared__ int finite[REG_PEAK_THREADS / 64];
    const int n = blockIdx.x;
    if (keep) {                                                       // uniform over the workgroup
        const float p = peak[n];
        if (p != p) return;
    }
    const double* cn = C + (int64_t)n * U * U;
    const unsigned cells = (unsigned)U * (unsigned)U;
    rfp_best k = {0ull, 0xFFFFFFFFu};
    bool fin = false;
    for (unsigned i = threadIdx.x; i < cells; i += REG_PEAK_THREADS) {
        const double v = cn[i];
        k = rfp_max(k, rfp_best{rfp_ord(v), i});
        fin = fin || fabs(v) < (double)INFINITY;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k = rfp_max(k, rfp_best{__shfl_xor(k.o, o, 64), (unsigned)__shfl_xor((int)k.i, o, 64)});
    const bool wave_fin = __ballot(fin) != 0;
    if ((threadIdx.x & 63) == 0) bo[threadIdx.x >> 6] = k.o, bi[threadIdx.x >> 6] = k.i, finite[threadIdx.x >> 6] = wave_fin ? 1 : 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int any = 0;
#pragma unroll
    for (int w = 0; w < REG_PEAK_THREADS / 64; ++w) {
        k = rfp_max(k, rfp_best{bo[w], bi[w]});
        any |= finite[w];
    }
    const int py = ipeak[2 * n], px = ipeak[2 * n + 1];
    if (!any) {                                                       // no finite value on the fine grid: the integer peak
        shifts[2 * n] = (float)(double)py, shifts[2 * n + 1] = (float)(double)px;
        peak[n] = __builtin_nanf("");
        return;
    }
    const int r = U / 2;
    const int jy = (int)(k.i / (unsigned)U), jx = (int)(k.i - (unsigned)jy * (unsigned)U);
    const double c0 = cn[k.i];
    double dy = 0.0, dx = 0.0;
    if (jy > 0 && jy < U - 1) dy = reg_parabola(cn[k.i - U], c0, cn[k.i + U]);
    if (jx > 0 && jx < U - 1) dx = reg_parabola(cn[k.i - 1], c0, cn[k.i + 1]);
    shifts[2 * n] = (float)((double)py + ((double)(jy - r) + dy) / (double)u);
    shifts[2 * n + 1] = (float)((double)px + ((double)(jx - r) + dx) / (double)u);
    peak[n] = (float)c0;
}

extern "C" int cwfa_reg_fine_peak_f64(const double* C, const int* ipeak, int N, int U, int u, int keep, float* shifts, float* peak, void* stream) {
    CWFA_REQUIRE(C && ipeak && shifts && peak, CWFA_E_INVAL, "cwfa_reg_fine_peak_f64: null pointer");
    CWFA_REQUIRE(keep == 0 || keep == 1, CWFA_E_INVAL, "cwfa_reg_fine_peak_f64: keep is 0 or 1");
    CWFA_REQUIRE(N >= 0, CWFA_E_SHAPE, "cwfa_reg_fine_peak_f64: negative size");
    CWFA_REQUIRE(u >= 1, CWFA_E_INVAL, "cwfa_reg_fine_peak_f64: the factor is at least 1, got %d", u);
    CWFA_REQUIRE(U >= 3 && (U & 1) == 1 && U < (1 << 15), CWFA_E_SHAPE, "cwfa_reg_fine_peak_f64: the fine grid has 2 r + 1 points a side, 1 <= r < 2^14, got %d", U);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(C) | reinterpret_cast<uintptr_t>(shifts) | reinterpret_cast<uintptr_t>(ipeak)) & 7u) == 0 &&
                     (reinterpret_cast<uintptr_t>(peak) & 3u) == 0,
                 CWFA_E_ALIGN, "cwfa_reg_fine_peak_f64: C, shifts and ipeak must be 8-byte aligned, peak 4-byte aligned");
    if (N == 0) return CWFA_OK;
    hipLaunchKernelGGL(rfp_kernel, dim3((unsigned)N), dim3(REG_PEAK_THREADS), 0, (hipStream_t)stream, C, ipeak, U, u, keep, shifts, peak);
    CWFA_LAUNCH_CHECK("cwfa_reg_fine_peak_f64");
    return CWFA_OK;
}
