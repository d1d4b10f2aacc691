// Rigid registration of reconstructed volumes: the passes of section 26 carried to [N, D, H, W] stacks.  rocFFT
// (through torch.fft.rfftn) does the transforms and cwfa_reg_whiten_c64 the whitened cross-power (a bin is a bin in any dimension);
// the edge taper is the kernel of register_internal.h that the frames run at D = 1; here are its entry point for volumes, the peak
// (rpeak3_*, over the key and the parabola of register_internal.h) and the trilinear resampling (rshift3_*), the 2-D arithmetic plus
// one axis, spelled so that D = 1 gives the 2-D bits.  All offsets into a stack are 64-bit: 32 volumes of 96 x 512 x 512 are
// 3 * 2^28 elements.  Built with -ffp-contract=off; the counted operations use the __f*_rn intrinsics all the same.
#include <math.h>
#include "common.h"
#include "register_internal.h"

// what the three entry points ask of a volume: sides that stay ints with a margin, fewer than 2^31 voxels
static inline bool r3_sizes_ok(int D, int H, int W) {
    return D < (1 << 30) && H < (1 << 30) && W < (1 << 30) && (int64_t)D * H < ((int64_t)1 << 31) && (int64_t)D * H * W < ((int64_t)1 << 31);
}

// ------------------------------------------------------------------------------------------------ the window
// out[n,z,y,x] = fl(x[n,z,y,x] * fl(fl(wz[z] * wy[y]) * wx[x])): reg_window_kernel (register_internal.h), fp32 only.
extern "C" int cwfa_reg_window3d_f32(const float* x, int N, int D, int H, int W, int64_t vol_stride, const float* wz, const float* wy,
                                     const float* wx, float* out, void* stream) {
    CWFA_REQUIRE(x && wz && wy && wx && out, CWFA_E_INVAL, "cwfa_reg_window3d_f32: null pointer");
    CWFA_REQUIRE(N >= 0 && D >= 0 && H >= 0 && W >= 0, CWFA_E_SHAPE, "cwfa_reg_window3d_f32: negative size");
    CWFA_REQUIRE(r3_sizes_ok(D, H, W), CWFA_E_SHAPE, "cwfa_reg_window3d_f32: a volume of %d x %d x %d is too large", D, H, W);
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
    CWFA_REQUIRE(r3_sizes_ok(D, H, W), CWFA_E_SHAPE, "cwfa_reg_peak3d_f32: a volume of %d x %d x %d is too large", D, H, W);
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
// out[n,z] = fl(wz0 * p_0) + fl(wz1 * p_1) with iz = floorf(dz), fz = fl(dz - iz), (wz0, wz1) = (fl(1 - fz), fz) and p_r the plane
// z + iz + r of volume n resampled under (dy, dx) by rshift_pixels (register_internal.h: the bits of cwfa_reg_shift); a plane
// outside the volume holds `fill`; a plane of weight exactly 0 is neither read nor added (wz0 == 0 happens: a tiny negative dz has
// fl(dz - iz) == 1); a non-finite component fills the volume.
//
// A thread owns V consecutive voxels of a row and a segment of at most RSHIFT3_ZSEG planes, and walks z: p_1 of plane z IS p_0 of
// plane z + 1 (the same function of the same source plane), so it is kept in registers and a source plane is read once per
// segment -- (ZSEG + 1) / ZSEG of the stack in all, whichever XCD's L2 a workgroup lands on.  The segments of one (y, x) band have
// consecutive block indices, so they are in flight together and the plane two of them share is still in a cache.  The volumes are
// walked inside the kernel (blockIdx.y, + gridDim.y, ..).
#define RSHIFT3_ZSEG 16

template <int V>
__device__ __forceinline__ void rshift3_plane(const float* __restrict__ vol, int D, int H, int W, int zz, int y, int x0, float dy, float dx, int nearest,
                                              float fill, float (&acc)[V]) {
    if (zz < 0 || zz >= D) {
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = fill;
    } else {
        rshift_pixels<V, float>(vol + (int64_t)zz * H * W, H, W, y, x0, dy, dx, nearest, fill, acc);
    }
}

template <int V>
__global__ __launch_bounds__(256) void rshift3_kernel(const float* __restrict__ in, int N, int D, int H, int W, int64_t vs, const float* __restrict__ shifts,
                                                      int nearest, float fill, int nseg, int zseg, float* __restrict__ out) {
    typedef float fvec __attribute__((ext_vector_type(V)));
    const int Wv = W / V;                                             // V > 1: W is a multiple of V
    const int seg = (int)(blockIdx.x % (unsigned)nseg);
    const int64_t q = (int64_t)(blockIdx.x / (unsigned)nseg) * blockDim.x + threadIdx.x;
    if (q >= (int64_t)H * Wv) return;
    const int y = (int)(q / Wv), x0 = (int)(q - (int64_t)y * Wv) * V;
    const int z0 = seg * zseg, z1 = z0 + zseg < D ? z0 + zseg : D;
    const int64_t HW = (int64_t)H * W;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        float dz = shifts[3 * (int64_t)n], dy = shifts[3 * (int64_t)n + 1], dx = shifts[3 * (int64_t)n + 2];
        const float* vol = in + (int64_t)n * vs;
        float* o = out + (int64_t)n * D * HW + (int64_t)y * W + x0;
        if (!(fabsf(dz) < INFINITY) || !(fabsf(dy) < INFINITY) || !(fabsf(dx) < INFINITY)) {
            fvec r;
#pragma unroll
            for (int j = 0; j < V; ++j) r[j] = fill;
            for (int z = z0; z < z1; ++z) *reinterpret_cast<fvec*>(o + (int64_t)z * HW) = r;
            continue;
        }
        if (nearest) dz = rintf(dz);                                  // rshift_pixels rounds (dy, dx) itself
        const float izf = floorf(dz);
        const float fz = __fsub_rn(dz, izf);
        const int iz = (int)fminf(fmaxf(izf, -(float)(D + 1)), (float)(D + 1));   // beyond: every plane is outside whatever the value
        const float w0 = __fsub_rn(1.f, fz), w1 = fz;
        const bool use0 = w0 != 0.f, use1 = w1 != 0.f;                // never both false: fz == 0 gives w0 == 1
        float a[V] = {}, b[V] = {};                                   // the unused one of the two stays 0 and is not read
        if (use0) rshift3_plane<V>(vol, D, H, W, z0 + iz, y, x0, dy, dx, nearest, fill, a);
        for (int z = z0; z < z1; ++z) {
            if (use1) rshift3_plane<V>(vol, D, H, W, z + iz + 1, y, x0, dy, dx, nearest, fill, b);
            fvec r;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float t0 = __fmul_rn(w0, a[j]), t1 = __fmul_rn(w1, b[j]);
                r[j] = use0 ? (use1 ? __fadd_rn(t0, t1) : t0) : t1;
            }
            *reinterpret_cast<fvec*>(o + (int64_t)z * HW) = r;
            if (use0 && use1) {                                       // plane z + iz + 1 is the next step's first plane
#pragma unroll
                for (int j = 0; j < V; ++j) a[j] = b[j];
            } else if (use0 && z + 1 < z1) {
                rshift3_plane<V>(vol, D, H, W, z + 1 + iz, y, x0, dy, dx, nearest, fill, a);
            }
        }
    }
}

extern "C" int cwfa_reg_shift3d_f32(const float* in, int N, int D, int H, int W, int64_t vol_stride, const float* shifts, int mode, float fill,
                                    float* out, void* stream) {
    CWFA_REQUIRE(in && shifts && out, CWFA_E_INVAL, "cwfa_reg_shift3d_f32: null pointer");
    CWFA_REQUIRE(mode == 0 || mode == 1, CWFA_E_INVAL, "cwfa_reg_shift3d_f32: mode is 0 (bilinear) or 1 (nearest), got %d", mode);
    CWFA_REQUIRE(N >= 0 && D >= 0 && H >= 0 && W >= 0, CWFA_E_SHAPE, "cwfa_reg_shift3d_f32: negative size");
    // z + iz + 1 with |iz| <= D + 1 stays an int (and so along y and x, in rshift_pixels)
    CWFA_REQUIRE(r3_sizes_ok(D, H, W), CWFA_E_SHAPE, "cwfa_reg_shift3d_f32: a volume of %d x %d x %d is too large", D, H, W);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(shifts) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0, CWFA_E_ALIGN,
                 "cwfa_reg_shift3d_f32: fp32 data must be 4-byte aligned");
    CWFA_REQUIRE(out != in, CWFA_E_INVAL, "cwfa_reg_shift3d_f32: out must not alias the stack");
    if (N == 0 || D == 0 || H == 0 || W == 0) return CWFA_OK;
    const int64_t HW = (int64_t)H * W;
    CWFA_REQUIRE(vol_stride >= (int64_t)D * HW, CWFA_E_INVAL, "cwfa_reg_shift3d_f32: volume stride smaller than a volume");
    // 16-byte stores where W and out's base allow (every row of every volume then starts on 16 bytes); the loads take any alignment
    const bool v4 = (W & 3) == 0 && cwfa_aligned16(out);
    const int nseg = (D + RSHIFT3_ZSEG - 1) / RSHIFT3_ZSEG, zseg = (D + nseg - 1) / nseg;     // even segments: 96 planes are 6 x 16
    const int64_t gx = (((v4 ? HW >> 2 : HW) + 255) / 256) * nseg;   // <= D H W / 256 + D + nseg < 2^31
    const dim3 grid((unsigned)gx, reg_grid_y(gx, N, 65536));
    hipStream_t st = (hipStream_t)stream;
    if (v4) hipLaunchKernelGGL((rshift3_kernel<4>), grid, dim3(256), 0, st, in, N, D, H, W, vol_stride, shifts, mode, fill, nseg, zseg, out);
    else hipLaunchKernelGGL((rshift3_kernel<1>), grid, dim3(256), 0, st, in, N, D, H, W, vol_stride, shifts, mode, fill, nseg, zseg, out);
    CWFA_LAUNCH_CHECK("cwfa_reg_shift3d_f32");
    return CWFA_OK;
}
