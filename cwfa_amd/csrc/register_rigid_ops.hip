// Rigid registration of reconstructed volumes with a rotation about the optical axis: the table of block shifts
// of section 32 is fitted by "rotation about z + 3-D shift" and the volume is resampled once under that motion.  Here:
//   rrfit_*    the rigid fit of a block-shift table, float64, one thread per volume, fixed order, no atomics, and its composition
//              with the motion already applied to the measured volumes
//   rrigid3_*  the resampling: the in-plane displacement of a voxel from (c - 1, s), then the z walk of register_internal.h over
//              rshift_pixels<1>
// No trigonometric function is evaluated: (c, s) come out of the fit by a square root and two divisions, and c - 1 is always formed
// as -(s s) / (1 + c).  All offsets into a stack are 64-bit.  Built with -ffp-contract=off; the counted fp32 operations use the
// __f*_rn intrinsics all the same.  tests/register_rigid_ref.py is the numpy restatement.
#include <math.h>
#include "common.h"
#include "register_internal.h"

// ------------------------------------------------------------------------------------------------ the fit
// One thread per volume, everything float64, every sum over the blocks in order b = 0 .. B - 1 from 0.0 (a block of weight 0 is
// skipped), every product, sum, difference, quotient and square root rounded on its own; a = arms[b] (block centre - c0, (y, x)):
//   m = sum w;  am = (sum w a) / m;  sm = (sum w s) / m;  e = a - am;  f = e + (s_yx - sm_yx);
//   P = sum w (ey fy + ex fx);  Q = sum w (ey fx - ex fy);  r = sqrt(P P + Q Q);
//   (c, s) = (P / r, Q / r) where r > 0, P > 0 and both are finite, else (1, 0);  cm1 = -(s s) / (1 + c);
//   dz = sm_z;  dy = sm_y - (cm1 am_y - s am_x);  dx = sm_x - (s am_y + cm1 am_x).
// The weights live in `inlier` between the passes: the thread that wrote a byte reads it.
struct rrfit_result {
    double dz, dy, dx, c, s;
};

__device__ __forceinline__ double rr_cm1(double c, double s) { return -(s * s) / (1.0 + c); }

__device__ __forceinline__ bool rrfit_once(const float* __restrict__ s, const double* __restrict__ a, const unsigned char* w, int B, rrfit_result& f) {
    double m = 0.0, ay = 0.0, ax = 0.0, sz = 0.0, sy = 0.0, sx = 0.0;
    for (int b = 0; b < B; ++b) {
        if (!w[b]) continue;
        m = m + 1.0;
        ay = ay + a[2 * b], ax = ax + a[2 * b + 1];
        sz = sz + (double)s[3 * b], sy = sy + (double)s[3 * b + 1], sx = sx + (double)s[3 * b + 2];
    }
    if (!(m >= 1.0)) return false;
    ay = ay / m, ax = ax / m, sz = sz / m, sy = sy / m, sx = sx / m;
    double P = 0.0, Q = 0.0;
    for (int b = 0; b < B; ++b) {
        if (!w[b]) continue;
        const double ey = a[2 * b] - ay, ex = a[2 * b + 1] - ax;
        const double fy = ey + ((double)s[3 * b + 1] - sy), fx = ex + ((double)s[3 * b + 2] - sx);
        P = P + (ey * fy + ex * fx);
        Q = Q + (ey * fx - ex * fy);
    }
    const double r = __dsqrt_rn(P * P + Q * Q);
    f.c = 1.0, f.s = 0.0;
    if (r > 0.0 && P > 0.0) {
        const double c = P / r, sn = Q / r;
        if (fabs(c) < (double)INFINITY && fabs(sn) < (double)INFINITY) f.c = c, f.s = sn;
    }
    const double cm1 = rr_cm1(f.c, f.s);
    f.dz = sz;
    f.dy = sy - (cm1 * ay - f.s * ax);
    f.dx = sx - (f.s * ay + cm1 * ax);
    return true;
}

__global__ __launch_bounds__(64) void rrfit_kernel(const float* __restrict__ shifts, const float* __restrict__ peak, const double* __restrict__ arms, int N,
                                                   int B, double min_peak, double reject, const double* __restrict__ prior, double* __restrict__ params,
                                                   unsigned char* inlier) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* s = shifts + n * B * 3;
    unsigned char* w = inlier + n * B;
    for (int b = 0; b < B; ++b) {
        const double p = (double)peak[n * B + b];
        const bool fin = fabsf(s[3 * b]) < INFINITY && fabsf(s[3 * b + 1]) < INFINITY && fabsf(s[3 * b + 2]) < INFINITY;
        w[b] = fin && fabs(p) < (double)INFINITY && p >= min_peak ? 1 : 0;
    }
    rrfit_result f = {0.0, 0.0, 0.0, 1.0, 0.0};
    if (rrfit_once(s, arms, w, B, f)) {
        const double cm1 = rr_cm1(f.c, f.s);
        int left = 0, gone = 0;
        for (int b = 0; b < B; ++b) {
            if (!w[b]) continue;
            const double ay = arms[2 * b], ax = arms[2 * b + 1];
            const double rz = fabs((double)s[3 * b] - f.dz);
            const double ry = fabs((double)s[3 * b + 1] - (f.dy + (cm1 * ay - f.s * ax)));
            const double rx = fabs((double)s[3 * b + 2] - (f.dx + (f.s * ay + cm1 * ax)));
            const double ryx = ry > rx ? ry : rx;
            if ((rz > ryx ? rz : ryx) > reject) w[b] = 2, ++gone;     // marked, not yet dropped: the first weights may have to come back
            else ++left;
        }
        if (gone && left) {
            for (int b = 0; b < B; ++b) w[b] = w[b] == 1 ? 1 : 0;
            rrfit_once(s, arms, w, B, f);
        } else if (gone) {                                            // nothing left: the first fit and the first weights
            for (int b = 0; b < B; ++b) w[b] = w[b] ? 1 : 0;
        }
    }
    if (prior) {                                                      // total = prior o fit: R' R, R' d + d'
        const double* q = prior + 5 * n;
        const double cp = q[3], sp = q[4];
        const double C = cp * f.c - sp * f.s, S = sp * f.c + cp * f.s;
        const double h = __dsqrt_rn(C * C + S * S);
        const double cm1p = rr_cm1(cp, sp);
        const double dy = (f.dy + (cm1p * f.dy - sp * f.dx)) + q[1];
        const double dx = (f.dx + (sp * f.dy + cm1p * f.dx)) + q[2];
        f.dz = f.dz + q[0], f.dy = dy, f.dx = dx, f.c = C / h, f.s = S / h;
    }
    double* o = params + 5 * n;
    o[0] = f.dz, o[1] = f.dy, o[2] = f.dx, o[3] = f.c, o[4] = f.s;
}

extern "C" int cwfa_reg_fit_rigid_f64(const float* shifts, const float* peak, const double* arms, int N, int B, double min_peak, double reject,
                                      const double* prior, double* params, uint8_t* inlier, void* stream) {
    const char* fn = "cwfa_reg_fit_rigid_f64";
    CWFA_REQUIRE(shifts && peak && arms && params && inlier, CWFA_E_INVAL, "%s: null pointer", fn);
    CWFA_REQUIRE(N >= 0, CWFA_E_SHAPE, "%s: negative size", fn);
    CWFA_REQUIRE(B >= 1 && B <= REG_MAX_BLOCKS, CWFA_E_SHAPE, "%s: 1 to %d blocks are expected, got %d", fn, REG_MAX_BLOCKS, B);
    CWFA_REQUIRE(min_peak >= 0.0 && reject >= 0.0, CWFA_E_INVAL, "%s: min_peak and reject are not negative and not NaN", fn);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(arms) | reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(prior)) & 7u) == 0 &&
                     ((reinterpret_cast<uintptr_t>(shifts) | reinterpret_cast<uintptr_t>(peak)) & 3u) == 0,
                 CWFA_E_ALIGN, "%s: arms, params and prior must be 8-byte aligned, shifts and peak 4-byte aligned", fn);
    CWFA_REQUIRE(prior != params, CWFA_E_INVAL, "%s: params must not alias prior", fn);
    if (N == 0) return CWFA_OK;
    hipLaunchKernelGGL(rrfit_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, shifts, peak, arms, N, B, min_peak, reject, prior,
                       params, inlier);
    CWFA_LAUNCH_CHECK("cwfa_reg_fit_rigid_f64");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the resampling
// Per volume (dzf, dyf, dxf, sf) = the fp32 roundings of (dz, dy, dx, s) and cm1f = (float)(-(s s) / (1 + c)), formed in float64; per
// voxel py = (float)y - cy, px = (float)x - cx,
//   vy = fl(dyf + fl(fl(cm1f py) - fl(sf px))),  vx = fl(dxf + fl(fl(sf py) + fl(cm1f px)))
// and out[n,z,y,x] = step 7 of section 30.1 under (dzf, vy, vx).  A parameter that is not finite fills the volume.
//
// (vy, vx) does not depend on z, nor does anything rshift_pixels derives from it -- the floors, the four weights, the tap offsets,
// the inside / outside decisions.  So this is the walk of register_internal.h: a thread forms its V vectors once per volume, a source
// plane is resampled by rshift_pixels<1> per voxel under (vy[j], vx[j]), and a voxel whose vector overflowed is masked (it fills, as
// in rbwarp_kernel).
template <int V>
__global__ __launch_bounds__(256) void rrigid3_kernel(const float* __restrict__ in, int N, int D, int H, int W, int64_t vs, const double* __restrict__ params,
                                                      float cy, float cx, int nearest, float fill, int nseg, int zseg, float* __restrict__ out) {
    reg3_tile t;
    if (!reg3_tile_of<V>(D, H, W, nseg, zseg, t)) return;
    const int64_t HW = (int64_t)H * W;
    const float py = __fsub_rn((float)t.y, cy);
    float px[V];
#pragma unroll
    for (int j = 0; j < V; ++j) px[j] = __fsub_rn((float)(t.x0 + j), cx);
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const double* p = params + 5 * (int64_t)n;
        const double c = p[3], s = p[4];
        const float dz = (float)p[0], dyf = (float)p[1], dxf = (float)p[2], sf = (float)s, cm1f = (float)(-(s * s) / (1.0 + c));
        const float* vol = in + (int64_t)n * vs;
        float* o = out + (int64_t)n * D * HW + t.p;
        if (!(fabs(c) < (double)INFINITY) || !(fabsf(dz) < INFINITY) || !(fabsf(dyf) < INFINITY) || !(fabsf(dxf) < INFINITY) || !(fabsf(sf) < INFINITY) ||
            !(fabsf(cm1f) < INFINITY)) {
            reg3_fill<V>(o, HW, t.z0, t.z1, fill);
            continue;
        }
        float vy[V], vx[V];
        bool bad[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            vy[j] = __fadd_rn(dyf, __fsub_rn(__fmul_rn(cm1f, py), __fmul_rn(sf, px[j])));
            vx[j] = __fadd_rn(dxf, __fadd_rn(__fmul_rn(sf, py), __fmul_rn(cm1f, px[j])));
            bad[j] = !(fabsf(vy[j]) < INFINITY) || !(fabsf(vx[j]) < INFINITY);
        }
        reg3_walk<V>(o, D, HW, t.z0, t.z1, reg3_zsplit_of(dz, nearest, D), bad, fill, [&](int zz, float(&acc)[V]) {
            const float* plane = vol + (int64_t)zz * H * W;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float a[1];
                rshift_pixels<1, float>(plane, H, W, t.y, t.x0 + j, vy[j], vx[j], nearest, fill, a);
                acc[j] = a[0];
            }
        });
    }
}

extern "C" int cwfa_reg_rigid3d_f32(const float* in, int N, int D, int H, int W, int64_t vol_stride, const double* params, float cy, float cx, int mode,
                                    float fill, float* out, void* stream) {
    const char* fn = "cwfa_reg_rigid3d_f32";
    CWFA_REQUIRE(in && params && out, CWFA_E_INVAL, "%s: null pointer", fn);
    REG3_REQUIRE_MODE(fn, mode);
    CWFA_REQUIRE(fabsf(cy) < INFINITY && fabsf(cx) < INFINITY, CWFA_E_INVAL, "%s: the centre (%g, %g) is not finite", fn, (double)cy, (double)cx);
    REG3_REQUIRE_SIZES(fn, N, D, H, W);
    CWFA_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0 && (reinterpret_cast<uintptr_t>(params) & 7u) == 0,
                 CWFA_E_ALIGN, "%s: the volumes must be 4-byte aligned, params 8-byte aligned", fn);
    REG3_REQUIRE_STACK(fn, in, out, N, D, H, W, vol_stride);
    REG3_LAUNCH(rrigid3_kernel, N, D, H, W, out, (hipStream_t)stream, in, N, D, H, W, vol_stride, params, cy, cx, mode, fill);
    CWFA_LAUNCH_CHECK(fn);
    return CWFA_OK;
}

