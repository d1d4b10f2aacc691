// Rigid registration of reconstructed volumes: the passes of section 26 carried to [N, D, H, W] stacks.  rocFFT
// (through torch.fft.rfftn) does the transforms and cwfa_reg_whiten_c64 the whitened cross-power (a bin is a bin in any dimension);
// the edge taper is the kernel of register_internal.h that the frames run at D = 1; here are its entry point for volumes, the peak
// (rpeak3_*, over the key and the parabola of register_internal.h) and the trilinear resampling (rshift3_*): the z walk of
// register_internal.h over the 2-D arithmetic, spelled so that D = 1 gives the 2-D bits.  All offsets into a stack are 64-bit: 32
// volumes of 96 x 512 x 512 are 3 * 2^28 elements.  Built with -ffp-contract=off; the counted operations use the __f*_rn intrinsics
// all the same.
#include <math.h>
#include "common.h"
#include "register_internal.h"

// ------------------------------------------------------------------------------------------------ the window
// out[n,z,y,x] = fl(x[n,z,y,x] * fl(fl(wz[z] * wy[y]) * wx[x])): reg_window_kernel (register_internal.h), fp32 only.
extern "C" int cwfa_reg_window3d_f32(const float* x, int N, int D, int H, int W, int64_t vol_stride, const float* wz, const float* wy,
                                     const float* wx, float* out, void* stream) {
    CWFA_REQUIRE(x && wz && wy && wx && out, CWFA_E_INVAL, "cwfa_reg_window3d_f32: null pointer");
    REG3_REQUIRE_SIZES("cwfa_reg_window3d_f32", N, D, H, W);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wz) | reinterpret_cast<uintptr_t>(wy) | reinterpret_cast<uintptr_t>(wx) |
                   reinterpret_cast<uintptr_t>(out)) & 3u) == 0,
                 CWFA_E_ALIGN, "cwfa_reg_window3d_f32: fp32 data must be 4-byte aligned");
    if (N == 0 || D == 0 || H == 0 || W == 0) return CWFA_OK;
    const int64_t P = (int64_t)D * H * W;
    CWFA_REQUIRE(vol_stride >= P, CWFA_E_INVAL, "cwfa_reg_window3d_f32: volume stride smaller than a volume");
    CWFA_REQUIRE(out != x, CWFA_E_INVAL, "cwfa_reg_window3d_f32: out must not be the stack");
    const bool v4 = (W & 3) == 0 && (vol_stride & 3) == 0 && cwfa_aligned16(wx) && cwfa_aligned16(out) && cwfa_aligned16(x);
    reg_window_launch(x, false, N, D, H, W, vol_stride, wz, wy, wx, out, v4, (hipStream_t)stream);
    CWFA_LAUNCH_CHECK("cwfa_reg_window3d_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the peak
// One workgroup per volume.  Window index i (row-major from (-mz, -my, -mx)) reads c at the shifts modulo (D, H, W); the key and its
// order are reg_peak_key's (register_internal.h), the reduction is rpeak_kernel's (register_ops.hip): the maximum over a thread's
// indices, over the wave by shuffles, over the waves through the LDS, no atomics.  Thread 0 then reads the peak's six neighbours
// (modulo the sides: they may lie outside the window) and fits the three parabolas in float64.
struct rpeak3_pos {
    int sz, sy, sx, z, y, x;
};
// window index -> signed shift and the voxel it reads; |s| < side on every axis: the window fits the volume
__device__ __forceinline__ rpeak3_pos rpeak3_at(unsigned i, int D, int H, int W, int mz, int my, int mx) {
    const unsigned wh = 2u * (unsigned)my + 1u, ww = 2u * (unsigned)mx + 1u;
    const unsigned r = i / ww, pz = r / wh;
    rpeak3_pos p;
    p.sx = (int)(i - r * ww) - mx, p.sy = (int)(r - pz * wh) - my, p.sz = (int)pz - mz;
    p.z = p.sz < 0 ? p.sz + D : p.sz, p.y = p.sy < 0 ? p.sy + H : p.sy, p.x = p.sx < 0 ? p.sx + W : p.sx;
    return p;
}

__global__ __launch_bounds__(REG_PEAK_THREADS) void rpeak3_kernel(const float* __restrict__ c, int N, int D, int H, int W, int64_t vs, int mz, int my,
                                                                int mx, int subpixel, float* __restrict__ shifts, int* __restrict__ ipeak,
                                                                float* __restrict__ peak) {
    __shared__ rkey_t best[REG_PEAK_THREADS / 64];
    __shared__ int finite[REG_PEAK_THREADS / 64];
    const unsigned nwin = (2u * (unsigned)mz + 1u) * (2u * (unsigned)my + 1u) * (2u * (unsigned)mx + 1u);   // <= D * H * W < 2^31
    for (int n = blockIdx.x; n < N; n += gridDim.x) {                 // uniform over the workgroup
        const float* cn = c + (int64_t)n * vs;
        rkey_t k = 0;
        bool fin = false;
        for (unsigned i = threadIdx.x; i < nwin; i += REG_PEAK_THREADS) {
            const rpeak3_pos p = rpeak3_at(i, D, H, W, mz, my, mx);
            const float v = cn[((int64_t)p.z * H + p.y) * W + p.x];
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
        __syncthreads();                                              // the previous volume's reads of the LDS are done
        if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = k, finite[threadIdx.x >> 6] = wave_fin ? 1 : 0;
        __syncthreads();
        if (threadIdx.x != 0) continue;
        int any = 0;
#pragma unroll
        for (int w = 0; w < REG_PEAK_THREADS / 64; ++w) {
            k = best[w] > k ? best[w] : k;
            any |= finite[w];
        }
        float* s = shifts + 3 * (int64_t)n;
        int* ip = ipeak + 3 * (int64_t)n;
        if (!any) {                                                   // no finite value in the window
            s[0] = 0.f, s[1] = 0.f, s[2] = 0.f;
            ip[0] = 0, ip[1] = 0, ip[2] = 0;
            peak[n] = __builtin_nanf("");
            continue;
        }
        const unsigned i = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
        const rpeak3_pos p = rpeak3_at(i, D, H, W, mz, my, mx);
        auto at = [&](int z, int y, int x) { return cn[((int64_t)z * H + y) * W + x]; };
        const float c0 = at(p.z, p.y, p.x);
        double dz = 0.0, dy = 0.0, dx = 0.0;
        if (subpixel) {
            const int zm = p.z == 0 ? D - 1 : p.z - 1, zp = p.z + 1 == D ? 0 : p.z + 1;
            const int ym = p.y == 0 ? H - 1 : p.y - 1, yp = p.y + 1 == H ? 0 : p.y + 1;
            const int xm = p.x == 0 ? W - 1 : p.x - 1, xp = p.x + 1 == W ? 0 : p.x + 1;
            dz = reg_parabola((double)at(zm, p.y, p.x), (double)c0, (double)at(zp, p.y, p.x));
            dy = reg_parabola((double)at(p.z, ym, p.x), (double)c0, (double)at(p.z, yp, p.x));
            dx = reg_parabola((double)at(p.z, p.y, xm), (double)c0, (double)at(p.z, p.y, xp));
        }
        s[0] = (float)((double)p.sz + dz), s[1] = (float)((double)p.sy + dy), s[2] = (float)((double)p.sx + dx);
        ip[0] = p.sz, ip[1] = p.sy, ip[2] = p.sx;
        peak[n] = c0;
    }
}

extern "C" int cwfa_reg_peak3d_f32(const float* c, int N, int D, int H, int W, int64_t vol_stride, int mz, int my, int mx, int subpixel,
                                   float* shifts, int* ipeak, float* peak, void* stream) {
    CWFA_REQUIRE(c && shifts && ipeak && peak, CWFA_E_INVAL, "cwfa_reg_peak3d_f32: null pointer");
    CWFA_REQUIRE(subpixel == 0 || subpixel == 1, CWFA_E_INVAL, "cwfa_reg_peak3d_f32: subpixel is 0 or 1");
    CWFA_REQUIRE(N >= 0 && D >= 0 && H >= 0 && W >= 0 && mz >= 0 && my >= 0 && mx >= 0, CWFA_E_SHAPE, "cwfa_reg_peak3d_f32: negative size");
    CWFA_REQUIRE(reg3_sizes_ok(D, H, W), CWFA_E_SHAPE, "cwfa_reg_peak3d_f32: a volume of %d x %d x %d is too large", D, H, W);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(shifts) | reinterpret_cast<uintptr_t>(ipeak) |
                   reinterpret_cast<uintptr_t>(peak)) & 3u) == 0,
                 CWFA_E_ALIGN, "cwfa_reg_peak3d_f32: c, shifts, ipeak and peak must be 4-byte aligned");
    if (N == 0 || D == 0 || H == 0 || W == 0) return CWFA_OK;
    // 2 m + 1 <= side on every axis, so the window holds at most D * H * W < 2^31 entries
    CWFA_REQUIRE(2 * (int64_t)mz + 1 <= D && 2 * (int64_t)my + 1 <= H && 2 * (int64_t)mx + 1 <= W, CWFA_E_SHAPE,
                 "cwfa_reg_peak3d_f32: the search window (%lld x %lld x %lld) is wider than the %d x %d x %d volume", 2 * (long long)mz + 1,
                 2 * (long long)my + 1, 2 * (long long)mx + 1, D, H, W);
    CWFA_REQUIRE(vol_stride >= (int64_t)D * H * W, CWFA_E_INVAL, "cwfa_reg_peak3d_f32: volume stride smaller than a volume");
    const unsigned gx = N < 65536 ? (unsigned)N : 65536u;             // a workgroup walks the volumes gridDim.x apart
    hipLaunchKernelGGL(rpeak3_kernel, dim3(gx), dim3(REG_PEAK_THREADS), 0, (hipStream_t)stream, c, N, D, H, W, vol_stride, mz, my, mx, subpixel, shifts,
                       ipeak, peak);
    CWFA_LAUNCH_CHECK("cwfa_reg_peak3d_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the resampling
// The walk of register_internal.h under one vector (dz, dy, dx) per volume: a source plane is resampled by rshift_pixels<V> under
// (dy, dx) and no voxel is masked.  A non-finite component fills the volume.
template <int V>
__global__ __launch_bounds__(256) void rshift3_kernel(const float* __restrict__ in, int N, int D, int H, int W, int64_t vs, const float* __restrict__ shifts,
                                                      int nearest, float fill, int nseg, int zseg, float* __restrict__ out) {
    reg3_tile t;
    if (!reg3_tile_of<V>(D, H, W, nseg, zseg, t)) return;
    const int64_t HW = (int64_t)H * W;
    const bool none[V] = {};
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const float dz = shifts[3 * (int64_t)n], dy = shifts[3 * (int64_t)n + 1], dx = shifts[3 * (int64_t)n + 2];
        const float* vol = in + (int64_t)n * vs;
        float* o = out + (int64_t)n * D * HW + t.p;
        if (!(fabsf(dz) < INFINITY) || !(fabsf(dy) < INFINITY) || !(fabsf(dx) < INFINITY)) {
            reg3_fill<V>(o, HW, t.z0, t.z1, fill);
            continue;
        }
        reg3_walk<V>(o, D, HW, t.z0, t.z1, reg3_zsplit_of(dz, nearest, D), none, fill, [&](int zz, float(&acc)[V]) {
            rshift_pixels<V, float>(vol + (int64_t)zz * H * W, H, W, t.y, t.x0, dy, dx, nearest, fill, acc);
        });
    }
}

extern "C" int cwfa_reg_shift3d_f32(const float* in, int N, int D, int H, int W, int64_t vol_stride, const float* shifts, int mode, float fill,
                                    float* out, void* stream) {
    const char* fn = "cwfa_reg_shift3d_f32";
    CWFA_REQUIRE(in && shifts && out, CWFA_E_INVAL, "%s: null pointer", fn);
    REG3_REQUIRE_MODE(fn, mode);
    REG3_REQUIRE_SIZES(fn, N, D, H, W);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(shifts) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0, CWFA_E_ALIGN,
                 "%s: fp32 data must be 4-byte aligned", fn);
    REG3_REQUIRE_STACK(fn, in, out, N, D, H, W, vol_stride);
    REG3_LAUNCH(rshift3_kernel, N, D, H, W, out, (hipStream_t)stream, in, N, D, H, W, vol_stride, shifts, mode, fill);
    CWFA_LAUNCH_CHECK(fn);
    return CWFA_OK;
}

