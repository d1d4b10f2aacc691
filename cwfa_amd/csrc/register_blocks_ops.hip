// Piecewise-rigid registration of reconstructed volumes: a volume is cut into a grid of blocks, every block is
// registered by the phase correlation of section 30 (the batch of blocks is to a volume what the batch of views is to a frame: the
// transforms, cwfa_reg_whiten_c64 and cwfa_reg_peak3d_f32 run unchanged), the table of block shifts is cleaned once, interpolated
// trilinearly between the block centres and the volume is resampled once under a displacement that differs per voxel.  Here:
//   rbwin_*    cuts and tapers the blocks of every volume in one read of each block
//   rbfill_*   the clean-up of the shift table, one thread per node, float64, fixed order, no atomics
//   rbwarp_*   the resampling: the node interpolation per voxel and step 7 of section 30.1 through rshift_pixels<1>, over the tile, the
//              z split, the blend and the launch geometry of register_internal.h
// The block origins are a HOST table, checked here and handed to the kernel in its arguments (the form of the centre table of
// register_views_ops.hip): what a kernel indexes with is what was checked.  All offsets into a stack are 64-bit.  Built with
// -ffp-contract=off; the counted operations use the __f*_rn intrinsics all the same.  tests/register_blocks_ref.py is the numpy
// restatement.
#include <math.h>
#include "common.h"
#include "register_internal.h"

#define RB_ORIGINS 256                // origins per axis that one launch carries in its arguments

// g_a >= 1 and gz gy gx <= REG_MAX_BLOCKS, without overflow
static inline bool rb_grid_ok(int gz, int gy, int gx) {
    return gz >= 1 && gy >= 1 && gx >= 1 && gz <= REG_MAX_BLOCKS && gy <= REG_MAX_BLOCKS && gx <= REG_MAX_BLOCKS && (int64_t)gz * gy * gx <= REG_MAX_BLOCKS;
}

// ------------------------------------------------------------------------------------------------ the cut and the taper
// out[n,b,z,y,x] = fl(x[n, oz + z, oy + y, ox + x] * fl(fl(wz[z] * wy[y]) * wx[x])), b = (iz gy + iy) gx + ix.  A thread owns V voxels of
// a block's row, keeps their window product and walks the volumes blockIdx.z, blockIdx.z + gridDim.z, ..; blockIdx.y is the block
// within the launch's part of the grid (the whole grid unless an axis has more than RB_ORIGINS blocks).  A block starts anywhere:
// the V source voxels are one load of element alignment; every origin was checked to keep the block inside the volume.
struct RbOrigins {
    int o[3][RB_ORIGINS];
};

template <int V>
__global__ __launch_bounds__(256) void rbwin_kernel(const float* __restrict__ x, int N, int H, int W, int64_t vs, const RbOrigins og, int cz, int cy,
                                                    int cx, int fz, int fy, int fx, int gy, int gx, int64_t B, int bz, int by, int bx,
                                                    const float* __restrict__ wz, const float* __restrict__ wy, const float* __restrict__ wx,
                                                    float* __restrict__ out) {
    typedef float fvec __attribute__((ext_vector_type(V)));
    const int Wv = bx / V;                                            // V > 1: bx is a multiple of V
    const int q = blockIdx.x * blockDim.x + threadIdx.x;              // bz * by * bx < 2^31
    if (q >= bz * by * Wv) return;
    const int row = q / Wv, x0 = (q - row * Wv) * V;
    const int z = row / by, y = row - z * by;
    const int l = blockIdx.y;                                         // < cz * cy * cx
    const int lr = l / cx, lx = l - lr * cx, lz = lr / cy, ly = lr - lz * cy;
    const int64_t b = ((int64_t)(fz + lz) * gy + (fy + ly)) * gx + (fx + lx);
    float w[V];
    {
        const float a = __fmul_rn(wz[z], wy[y]);
#pragma unroll
        for (int j = 0; j < V; ++j) w[j] = __fmul_rn(a, wx[x0 + j]);
    }
    const int64_t p = ((int64_t)(og.o[0][lz] + z) * H + (og.o[1][ly] + y)) * W + og.o[2][lx] + x0;
    const int64_t P = (int64_t)bz * by * bx;
    const int64_t o = b * P + (int64_t)row * bx + x0;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        rshift_span<float, V> sp;
        __builtin_memcpy(&sp, x + (int64_t)n * vs + p, sizeof(sp));
        fvec r;
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = __fmul_rn(sp.v[j], w[j]);
        *reinterpret_cast<fvec*>(out + (int64_t)n * B * P + o) = r;
    }
}

extern "C" int cwfa_reg_window_blocks3d_f32(const float* x, int N, int D, int H, int W, int64_t vol_stride, const int32_t* origins, int gz, int gy,
                                            int gx, int bz, int by, int bx, const float* wz, const float* wy, const float* wx, float* out,
                                            void* stream) {
    const char* fn = "cwfa_reg_window_blocks3d_f32";
    CWFA_REQUIRE(x && origins && wz && wy && wx && out, CWFA_E_INVAL, "%s: null pointer", fn);
    REG3_REQUIRE_SIZES(fn, N, D, H, W);
    CWFA_REQUIRE(rb_grid_ok(gz, gy, gx), CWFA_E_SHAPE, "%s: a grid of %d x %d x %d: every axis at least 1, at most %d blocks", fn, gz, gy, gx,
                 REG_MAX_BLOCKS);
    CWFA_REQUIRE(bz >= 1 && by >= 1 && bx >= 1 && bz <= D && by <= H && bx <= W, CWFA_E_SHAPE,
                 "%s: a block of %d x %d x %d does not fit the %d x %d x %d volume", fn, bz, by, bx, D, H, W);
    const int g[3] = {gz, gy, gx}, b[3] = {bz, by, bx}, S[3] = {D, H, W};
    for (int a = 0, k = 0; a < 3; ++a)
        for (int i = 0; i < g[a]; ++i, ++k)
            CWFA_REQUIRE(origins[k] >= 0 && origins[k] <= S[a] - b[a], CWFA_E_INVAL, "%s: origin %d of axis %d (%d) puts the block outside the volume", fn,
                         i, a, origins[k]);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wz) | reinterpret_cast<uintptr_t>(wy) | reinterpret_cast<uintptr_t>(wx) |
                   reinterpret_cast<uintptr_t>(out)) & 3u) == 0,
                 CWFA_E_ALIGN, "%s: fp32 data must be 4-byte aligned", fn);
    CWFA_REQUIRE(vol_stride >= (int64_t)D * H * W, CWFA_E_INVAL, "%s: volume stride smaller than a volume", fn);
    CWFA_REQUIRE(out != x, CWFA_E_INVAL, "%s: out must not be the stack", fn);
    if (N == 0) return CWFA_OK;
    const bool v4 = (bx & 3) == 0 && cwfa_aligned16(out);             // 16-byte stores: every row of every block then starts on 16 bytes
    const int64_t B = (int64_t)gz * gy * gx;
    const int64_t nx = (((int64_t)bz * by * bx >> (v4 ? 2 : 0)) + 255) / 256;
    hipStream_t st = (hipStream_t)stream;
    // one launch, unless an axis has more origins than the arguments carry
    for (int fz = 0; fz < gz; fz += RB_ORIGINS)
        for (int fy = 0; fy < gy; fy += RB_ORIGINS)
            for (int fx = 0; fx < gx; fx += RB_ORIGINS) {
                const int cz = gz - fz < RB_ORIGINS ? gz - fz : RB_ORIGINS, cy = gy - fy < RB_ORIGINS ? gy - fy : RB_ORIGINS,
                          cx = gx - fx < RB_ORIGINS ? gx - fx : RB_ORIGINS;
                RbOrigins og;
                for (int i = 0; i < RB_ORIGINS; ++i) {
                    og.o[0][i] = i < cz ? origins[fz + i] : 0;
                    og.o[1][i] = i < cy ? origins[gz + fy + i] : 0;
                    og.o[2][i] = i < cx ? origins[gz + gy + fx + i] : 0;
                }
                const int64_t nb = (int64_t)cz * cy * cx;             // <= REG_MAX_BLOCKS
                const dim3 grid((unsigned)nx, (unsigned)nb, reg_grid_y(nx * nb, N, 65536));
                if (v4)
                    hipLaunchKernelGGL((rbwin_kernel<4>), grid, dim3(256), 0, st, x, N, H, W, vol_stride, og, cz, cy, cx, fz, fy, fx, gy, gx, B, bz, by, bx,
                                       wz, wy, wx, out);
                else
                    hipLaunchKernelGGL((rbwin_kernel<1>), grid, dim3(256), 0, st, x, N, H, W, vol_stride, og, cz, cy, cx, fz, fy, fx, gy, gx, B, bz, by, bx,
                                       wz, wy, wx, out);
                CWFA_LAUNCH_CHECK("cwfa_reg_window_blocks3d_f32");
            }
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the clean-up of the shift table
// A node is an inlier when its peak is finite and >= min_peak, its three components are finite and (dev) |s_c - base_c| <= max_dev_c,
// compared in float64.  An inlier keeps its bits; an outlier takes per component the float64 mean of the inliers among its 26 grid
// neighbours -- visited row-major over (dz, dy, dx) in {-1, 0, 1}^3, z slowest, status read from the input -- rounded once, or base[n]
// where it has none.  One thread per node.
struct RbDev {
    double m[3];
};

__device__ __forceinline__ bool rbfill_inlier(const float* __restrict__ s, float pk, const float* __restrict__ base, double min_peak, int dev,
                                              const RbDev& md) {
    if (!(fabsf(pk) < INFINITY) || !((double)pk >= min_peak)) return false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (!(fabsf(s[c]) < INFINITY)) return false;
        if (dev && !(fabs((double)s[c] - (double)base[c]) <= md.m[c])) return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void rbfill_kernel(const float* __restrict__ shifts, const float* __restrict__ peak, const float* __restrict__ base,
                                                     int64_t NB, int gz, int gy, int gx, double min_peak, int dev, const RbDev md,
                                                     float* __restrict__ field, unsigned char* __restrict__ inlier) {
    const int B = gz * gy * gx;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < NB; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = q / B;
        const int b = (int)(q - n * B);
        const float* sn = shifts + 3 * n * B;
        const float* pn = peak + n * B;
        const float* bn = base + 3 * n;
        const bool in = rbfill_inlier(sn + 3 * b, pn[b], bn, min_peak, dev, md);
        inlier[q] = in ? 1 : 0;
        float r[3];
        if (in) {
            r[0] = sn[3 * b], r[1] = sn[3 * b + 1], r[2] = sn[3 * b + 2];
        } else {
            const int r2 = b / gx, ix = b - r2 * gx, iz = r2 / gy, iy = r2 - iz * gy;
            double sum[3] = {0.0, 0.0, 0.0};
            int cnt = 0;
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int z = iz + dz, y = iy + dy, x = ix + dx;
                        if ((dz == 0 && dy == 0 && dx == 0) || z < 0 || z >= gz || y < 0 || y >= gy || x < 0 || x >= gx) continue;
                        const int nb = (z * gy + y) * gx + x;
                        if (!rbfill_inlier(sn + 3 * nb, pn[nb], bn, min_peak, dev, md)) continue;
                        sum[0] += (double)sn[3 * nb], sum[1] += (double)sn[3 * nb + 1], sum[2] += (double)sn[3 * nb + 2];
                        ++cnt;
                    }
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = cnt ? (float)(sum[c] / (double)cnt) : bn[c];
        }
        field[3 * q] = r[0], field[3 * q + 1] = r[1], field[3 * q + 2] = r[2];
    }
}

extern "C" int cwfa_reg_field_fill(const float* shifts, const float* peak, const float* base, int N, int gz, int gy, int gx, double min_peak,
                                   const double* max_dev, float* field, unsigned char* inlier, void* stream) {
    const char* fn = "cwfa_reg_field_fill";
    CWFA_REQUIRE(shifts && peak && base && field && inlier, CWFA_E_INVAL, "%s: null pointer", fn);
    CWFA_REQUIRE(N >= 0, CWFA_E_SHAPE, "%s: negative size", fn);
    CWFA_REQUIRE(rb_grid_ok(gz, gy, gx), CWFA_E_SHAPE, "%s: a grid of %d x %d x %d: every axis at least 1, at most %d blocks", fn, gz, gy, gx,
                 REG_MAX_BLOCKS);
    CWFA_REQUIRE(min_peak == min_peak, CWFA_E_INVAL, "%s: min_peak is NaN", fn);
    RbDev md = {{0.0, 0.0, 0.0}};
    if (max_dev)
        for (int c = 0; c < 3; ++c) {
            CWFA_REQUIRE(max_dev[c] >= 0.0, CWFA_E_INVAL, "%s: max_dev[%d] = %g is negative or NaN", fn, c, max_dev[c]);
            md.m[c] = max_dev[c];
        }
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(shifts) | reinterpret_cast<uintptr_t>(peak) | reinterpret_cast<uintptr_t>(base) |
                   reinterpret_cast<uintptr_t>(field)) & 3u) == 0,
                 CWFA_E_ALIGN, "%s: shifts, peak, base and field must be 4-byte aligned", fn);
    CWFA_REQUIRE(field != shifts, CWFA_E_INVAL, "%s: field must not be the shift table (a neighbour's status is read from the input)", fn);
    if (N == 0) return CWFA_OK;
    const int64_t NB = (int64_t)N * gz * gy * gx;
    const int64_t blocks = (NB + 255) / 256;
    hipLaunchKernelGGL(rbfill_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, (hipStream_t)stream, shifts, peak, base, NB, gz, gy,
                       gx, min_peak, max_dev ? 1 : 0, md, field, inlier);
    CWFA_LAUNCH_CHECK("cwfa_reg_field_fill");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the warp
// out[n,z,y,x] = step 7 of section 30.1 under the voxel's own (dz, dy, dx), the trilinear interpolation of the node table
// field[n] [gz, gy, gx, 3] with the axis tables (idx, t): lerp(a, b, t) = a where t == 0, else fl(a + fl(t * fl(b - a))), along x first
// (four times), then y (twice), then z; node i + 1 is not read where t == 0.  The resampling of a voxel is rshift_pixels<1> on planes
// z + floor(dz) and the next one under the z split and the blend of register_internal.h, whose tile and launch geometry the kernel
// takes too.
//
// The vector changes with z, so no resampled plane can be carried and the kernel walks its segment itself.  The x and y lerps of a
// node plane do not depend on z, so a thread keeps them for node planes iz and iz + 1 (2 x 3 V registers) and forms them again only
// where idxz steps; per output plane only the z lerp and the resampling are left.  The node table (at most 48 KB a volume) is read
// through the caches: the 8 nodes around a thread's voxels are shared by the whole workgroup almost everywhere.  Table indices are
// clamped to the grid before they index anything.
__device__ __forceinline__ float rb_lerp(float a, float b, float t) { return t == 0.f ? a : __fadd_rn(a, __fmul_rn(t, __fsub_rn(b, a))); }

// the (y, x) interpolation of node plane nz at the V voxels: Y[j][c]
template <int V>
__device__ __forceinline__ void rbwarp_plane(const float* __restrict__ fn, int nz, int gy, int gx, int iy, float ty, const int (&ix)[V],
                                             const float (&tx)[V], float (&Y)[V][3]) {
    const float* r0 = fn + 3 * ((int64_t)nz * gy + iy) * gx;
    const float* r1 = r0 + 3 * (int64_t)gx;                           // read where ty != 0 only: iy + 1 < gy there
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float* a = r0 + 3 * ix[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) Y[j][c] = tx[j] == 0.f ? a[c] : rb_lerp(a[c], a[3 + c], tx[j]);
        if (ty != 0.f) {
            const float* b = r1 + 3 * ix[j];
#pragma unroll
            for (int c = 0; c < 3; ++c) Y[j][c] = rb_lerp(Y[j][c], tx[j] == 0.f ? b[c] : rb_lerp(b[c], b[3 + c], tx[j]), ty);
        }
    }
}

// plane zz of the volume resampled at (y, x) under (dy, dx); a plane outside the volume holds `fill`
__device__ __forceinline__ float rbwarp_tap(const float* __restrict__ vol, int D, int H, int W, int zz, int y, int x, float dy, float dx, int nearest,
                                            float fill) {
    if (zz < 0 || zz >= D) return fill;
    float acc[1];
    rshift_pixels<1, float>(vol + (int64_t)zz * H * W, H, W, y, x, dy, dx, nearest, fill, acc);
    return acc[0];
}

template <int V>
__global__ __launch_bounds__(256) void rbwarp_kernel(const float* __restrict__ in, int N, int D, int H, int W, int64_t vs, const float* __restrict__ field,
                                                     int gz, int gy, int gx, const int* __restrict__ idxz, const float* __restrict__ tzt,
                                                     const int* __restrict__ idxy, const float* __restrict__ tyt, const int* __restrict__ idxx,
                                                     const float* __restrict__ txt, int nearest, float fill, int nseg, int zseg,
                                                     float* __restrict__ out) {
    typedef float fvec __attribute__((ext_vector_type(V)));
    reg3_tile t;
    if (!reg3_tile_of<V>(D, H, W, nseg, zseg, t)) return;
    const int y = t.y, x0 = t.x0;
    const int64_t HW = (int64_t)H * W;
    // the tables' entries of this thread, clamped to the grid; where idx is the last node, t is 0 by construction and is made so
    int iy = idxy[y];
    iy = iy < 0 ? 0 : (iy > gy - 1 ? gy - 1 : iy);
    const float ty = iy == gy - 1 ? 0.f : tyt[y];
    int ix[V];
    float tx[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        int i = idxx[x0 + j];
        i = i < 0 ? 0 : (i > gx - 1 ? gx - 1 : i);
        ix[j] = i, tx[j] = i == gx - 1 ? 0.f : txt[x0 + j];
    }
    const int64_t B3 = 3 * (int64_t)gz * gy * gx;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const float* fn = field + (int64_t)n * B3;
        const float* vol = in + (int64_t)n * vs;
        float* o = out + (int64_t)n * D * HW + t.p;
        float Y0[V][3], Y1[V][3];
        int cur = -1;
        bool have1 = false;
        for (int z = t.z0; z < t.z1; ++z) {
            int iz = idxz[z];
            iz = iz < 0 ? 0 : (iz > gz - 1 ? gz - 1 : iz);
            const float tz = iz == gz - 1 ? 0.f : tzt[z];
            if (iz != cur) {
                rbwarp_plane<V>(fn, iz, gy, gx, iy, ty, ix, tx, Y0);
                cur = iz, have1 = false;
            }
            if (tz != 0.f && !have1) {
                rbwarp_plane<V>(fn, iz + 1, gy, gx, iy, ty, ix, tx, Y1);
                have1 = true;
            }
            fvec r;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float dz = tz == 0.f ? Y0[j][0] : rb_lerp(Y0[j][0], Y1[j][0], tz);
                const float dy = tz == 0.f ? Y0[j][1] : rb_lerp(Y0[j][1], Y1[j][1], tz);
                const float dx = tz == 0.f ? Y0[j][2] : rb_lerp(Y0[j][2], Y1[j][2], tz);
                if (!(fabsf(dz) < INFINITY) || !(fabsf(dy) < INFINITY) || !(fabsf(dx) < INFINITY)) {
                    r[j] = fill;
                    continue;
                }
                const reg3_zsplit s = reg3_zsplit_of(dz, nearest, D);
                float p0 = 0.f, p1 = 0.f;
                if (s.use0) p0 = rbwarp_tap(vol, D, H, W, z + s.iz, y, x0 + j, dy, dx, nearest, fill);
                if (s.use1) p1 = rbwarp_tap(vol, D, H, W, z + s.iz + 1, y, x0 + j, dy, dx, nearest, fill);
                r[j] = reg3_blend(s, p0, p1);
            }
            *reinterpret_cast<fvec*>(o + (int64_t)z * HW) = r;
        }
    }
}

extern "C" int cwfa_reg_warp3d_f32(const float* in, int N, int D, int H, int W, int64_t vol_stride, const float* field, int gz, int gy, int gx,
                                   const int32_t* idxz, const float* tz, const int32_t* idxy, const float* ty, const int32_t* idxx, const float* tx,
                                   int mode, float fill, float* out, void* stream) {
    const char* fn = "cwfa_reg_warp3d_f32";
    CWFA_REQUIRE(in && field && idxz && tz && idxy && ty && idxx && tx && out, CWFA_E_INVAL, "%s: null pointer", fn);
    REG3_REQUIRE_MODE(fn, mode);
    REG3_REQUIRE_SIZES(fn, N, D, H, W);
    CWFA_REQUIRE(rb_grid_ok(gz, gy, gx), CWFA_E_SHAPE, "%s: a grid of %d x %d x %d: every axis at least 1, at most %d blocks", fn, gz, gy, gx,
                 REG_MAX_BLOCKS);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(field) | reinterpret_cast<uintptr_t>(idxz) | reinterpret_cast<uintptr_t>(tz) |
                   reinterpret_cast<uintptr_t>(idxy) | reinterpret_cast<uintptr_t>(ty) | reinterpret_cast<uintptr_t>(idxx) | reinterpret_cast<uintptr_t>(tx) |
                   reinterpret_cast<uintptr_t>(out)) & 3u) == 0,
                 CWFA_E_ALIGN, "%s: the volumes, the field and the tables must be 4-byte aligned", fn);
    REG3_REQUIRE_STACK(fn, in, out, N, D, H, W, vol_stride);
    REG3_LAUNCH(rbwarp_kernel, N, D, H, W, out, (hipStream_t)stream, in, N, D, H, W, vol_stride, field, gz, gy, gx, idxz, tz, idxy, ty, idxx, tx, mode, fill);
    CWFA_LAUNCH_CHECK(fn);
    return CWFA_OK;
}

