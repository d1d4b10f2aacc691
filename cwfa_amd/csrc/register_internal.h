// What the registration kernels share (register_ops.hip: frames; register_views_ops.hip: lenslet views; register3d_ops.hip: volumes;
// register_blocks_ops.hip: blocks of volumes; register_rigid_ops.hip: volumes that turn).
// One definition of each, so that a frame is a volume of one plane by construction and not by a copy kept in step:
//   the grid rule of the kernels whose threads walk the items                                         reg_grid_y
//   the edge taper over [N, D, H, W], D = 1 and no wz for frames                                      reg_window_kernel
//   the order of the integer peak's keys and the float64 parabola                                     reg_peak_key, reg_parabola
//   the arithmetic of step 7 of DESIGN.md section 26.1 for V consecutive pixels of a row              rshift_pixels
//   the store form of the two 2-D resampling entry points                                             reg_store_width
//   the size rule of a volume and the block limit of a grid                                           reg3_sizes_ok, REG_MAX_BLOCKS
//   the checks and the launch geometry of the three entry points that resample volumes                REG3_REQUIRE_*, REG3_LAUNCH
//   a thread's voxels and z segment, the split of dz, the blend of two planes, the segment fill       reg3_tile_of, reg3_zsplit_of, ..
//   the walk over a segment that carries a resampled plane from one output plane to the next          reg3_walk
#pragma once
#include <math.h>
#include <type_traits>
#include "common.h"

typedef unsigned long long rkey_t;

// blocks along y for a kernel whose threads walk the frames: about `target` blocks in all, the per-pixel values reused over N / gy
// frames.  The window and the resampling keep a few words per thread and take many blocks (an even tail); the whitening keeps a
// plane of weights and takes one block row where the bins alone fill the chip, so that the plane is read once.
static inline unsigned reg_grid_y(int64_t gx, int N, int64_t target) {
    int64_t gy = target / gx < 1 ? 1 : target / gx;
    gy = gy > 65535 ? 65535 : gy;
    return (unsigned)(gy > N ? N : gy);
}

// ------------------------------------------------------------------------------------------------ the window
// out[n,z,y,x] = fl(float(x[n,z,y,x]) * fl(a * wx[x])) with a = fl(wz[z] * wy[y]), or, PLANAR (frames: D = 1, wz null), wy[y] itself:
// no product by 1 is formed and no z is split off.  One read, one fp32 write.  A thread owns V elements of a row, keeps their
// window product and walks the items blockIdx.y, blockIdx.y + gridDim.y, ..  `stride` is the distance between items, in elements.
// (PLANAR is a compile-time flag because it measured: with `wz ? .. : ..` decided in the kernel the fp16 chunk of DESIGN.md
// section 26.3 took 0.095 ms beside 0.090 ms.)
template <int V, bool HALF, bool PLANAR>
__global__ __launch_bounds__(256) void reg_window_kernel(const void* __restrict__ x, int N, int D, int H, int W, int64_t stride,
                                                         const float* __restrict__ wz, const float* __restrict__ wy, const float* __restrict__ wx,
                                                         float* __restrict__ out) {
    using elem = std::conditional_t<HALF, _Float16, float>;
    typedef float fvec __attribute__((ext_vector_type(V)));
    typedef elem evec __attribute__((ext_vector_type(V)));
    const int Wv = W / V;                                             // V > 1: W is a multiple of V
    const int64_t rows = (int64_t)D * H;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= rows * Wv) return;
    const int64_t row = q / Wv;                                       // z * H + y < 2^31
    const int x0 = (int)(q - row * Wv) * V;
    const int z = PLANAR ? 0 : (int)((unsigned)row / (unsigned)H), y = (int)row - z * H;
    const int64_t p = row * W + x0;
    const int64_t P = rows * W;
    float w[V];
    {
        const float a = PLANAR ? wy[y] : __fmul_rn(wz[z], wy[y]);
        const fvec b = *reinterpret_cast<const fvec*>(wx + x0);
#pragma unroll
        for (int j = 0; j < V; ++j) w[j] = __fmul_rn(a, b[j]);
    }
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const evec v = *reinterpret_cast<const evec*>(reinterpret_cast<const elem*>(x) + (int64_t)n * stride + p);
        fvec r;
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = __fmul_rn((float)v[j], w[j]);
        *reinterpret_cast<fvec*>(out + (int64_t)n * P + p) = r;
    }
}

// the launch of both entry points, whose checks have been made: D * H * W < 2^31, `v4` where 16-byte (fp16: 8-byte) accesses are
// allowed; a null wz is the frames' form (D = 1), fp16 is theirs alone
static inline void reg_window_launch(const void* x, bool half, int N, int D, int H, int W, int64_t stride, const float* wz, const float* wy,
                                     const float* wx, float* out, bool v4, hipStream_t st) {
    const int64_t P = (int64_t)D * H * W;
    const int64_t gx = ((v4 ? P >> 2 : P) + 255) / 256;               // < 2^23
    const dim3 grid((unsigned)gx, reg_grid_y(gx, N, 65536));
#define REG_WINDOW_LAUNCH(V, HALF, PLANAR) \
    hipLaunchKernelGGL((reg_window_kernel<V, HALF, PLANAR>), grid, dim3(256), 0, st, x, N, D, H, W, stride, wz, wy, wx, out)
    if (wz) { if (v4) REG_WINDOW_LAUNCH(4, false, false); else REG_WINDOW_LAUNCH(1, false, false); }
    else if (v4) { if (half) REG_WINDOW_LAUNCH(4, true, true); else REG_WINDOW_LAUNCH(4, false, true); }
    else { if (half) REG_WINDOW_LAUNCH(1, true, true); else REG_WINDOW_LAUNCH(1, false, true); }
#undef REG_WINDOW_LAUNCH
}

// ------------------------------------------------------------------------------------------------ the peak's order and parabola
// key = ord(c + 0.0f) << 32 | (0xFFFFFFFF - i), the order of the detector (neuron_ops.hip): NaN has ord 0, ties go to the lowest
// window index i.  The peak kernels (rpeak_kernel, rpeak3_kernel) take the maximum key; they and the fine peak fit reg_parabola.
#define REG_PEAK_THREADS 256

__device__ __forceinline__ rkey_t reg_peak_key(float v, unsigned i) {
    unsigned u = __builtin_bit_cast(unsigned, v);
    u = u == 0x80000000u ? 0u : u;                                    // v + 0.0f
    const unsigned o = v != v ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
    return ((rkey_t)o << 32) | (rkey_t)(0xFFFFFFFFu - i);
}

// the offset of the vertex of the parabola through (-1, a), (0, b), (1, c), clamped to half a sample; 0 where b is no strict maximum
__device__ __forceinline__ double reg_parabola(double a, double b, double c) {
    const double den = (a - 2.0 * b) + c;
    double d = (0.5 * (a - c)) / den;
    if (!(den < 0.0) || !(fabs(d) <= 1.7976931348623157e308)) d = 0.0;
    return d < -0.5 ? -0.5 : (d > 0.5 ? 0.5 : d);
}

template <class T, int K>
struct rshift_span {
    T v[K];
};

// acc[j] = the resampled pixel (y, x0 + j), j = 0 .. V - 1, of the frame `src` [H, W] under the shift (dy, dx): the sum over the taps
// (0,0), (0,1), (1,0), (1,1) of w * src[y + iy + r, x + ix + c], iy = floorf(dy), fy = dy - iy, w = fl(wy_r * wx_c) with
// wy = (fl(1 - fy), fy): every weight and product rounded, the terms added in that order, a tap of weight exactly 0 neither read nor
// added (an integer shift copies bits), a tap outside the frame reads `fill`, a non-finite shift fills.  The V + 1 source pixels of
// either row start anywhere: inside the frame the span is one load of element alignment (the compiler makes it a vector load plus
// one element), at the borders element by element.
template <int V, class elem>
__device__ __forceinline__ void rshift_pixels(const elem* __restrict__ src, int H, int W, int y, int x0, float dy, float dx, int nearest, float fill,
                                              float (&acc)[V]) {
    if (!(fabsf(dy) < INFINITY) || !(fabsf(dx) < INFINITY)) {
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = fill;
    } else {
        if (nearest) dy = rintf(dy), dx = rintf(dx);
        const float iyf = floorf(dy), ixf = floorf(dx);
        const float fy = __fsub_rn(dy, iyf), fx = __fsub_rn(dx, ixf);
        // beyond +-(size + 1) every tap is outside whatever the value: clamp before the conversion to int
        const int iy = (int)fminf(fmaxf(iyf, -(float)(H + 1)), (float)(H + 1));
        const int ix = (int)fminf(fmaxf(ixf, -(float)(W + 1)), (float)(W + 1));
        const float wy[2] = {__fsub_rn(1.f, fy), fy}, wx[2] = {__fsub_rn(1.f, fx), fx};
        bool have = false;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const float w0 = __fmul_rn(wy[r], wx[0]), w1 = __fmul_rn(wy[r], wx[1]);
            if (w0 == 0.f && w1 == 0.f) continue;                 // the whole row of taps has weight 0: not read
            const int yy = y + iy + r;
            const bool row_in = yy >= 0 && yy < H;
            const elem* row = src + (int64_t)(row_in ? yy : 0) * W;
            float v[V + 1];
            const int xs = x0 + ix;
            if (V > 1 && row_in && xs >= 0 && xs + V < W) {       // the span lies inside the row: one unaligned vector load
                rshift_span<elem, V + 1> sp;
                __builtin_memcpy(&sp, row + xs, sizeof(sp));
#pragma unroll
                for (int j = 0; j <= V; ++j) v[j] = (float)sp.v[j];
            } else {
#pragma unroll
                for (int j = 0; j <= V; ++j) {
                    const int xx = xs + j;
                    const bool need = j < V ? (w0 != 0.f || (j > 0 && w1 != 0.f)) : w1 != 0.f;
                    v[j] = need && row_in && xx >= 0 && xx < W ? (float)row[xx] : fill;
                }
            }
            if (w0 != 0.f) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float t = __fmul_rn(w0, v[j]);
                    acc[j] = have ? __fadd_rn(acc[j], t) : t;
                }
                have = true;
            }
            if (w1 != 0.f) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float t = __fmul_rn(w1, v[j + 1]);
                    acc[j] = have ? __fadd_rn(acc[j], t) : t;
                }
                have = true;
            }
        }
        if (!have) {                                              // all four weights underflowed to 0
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the store form of the 2-D resampling
// Pixels per thread of rshift_kernel and rshiftl_kernel: 16-byte stores where W and out's base allow (eight fp16 or four fp32 pixels),
// four fp16 pixels (8 bytes) next, else one.  Every row of every frame then starts on that alignment; the loads take any.
static inline int reg_store_width(int dtype, int W, const void* out) {
    if (dtype == 1 && (W & 7) == 0 && cwfa_aligned16(out)) return 8;
    if ((W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (dtype ? 7u : 15u)) == 0) return 4;
    return 1;
}

// launches KERNEL<V, HALF> for the width `v` of reg_store_width on a grid of ceil(P / v / 256) x reg_grid_y blocks, P pixels a frame
#define REG_SHIFT_LAUNCH(KERNEL, v, dtype, P, N, st, ...)                                                                  \
    do {                                                                                                                   \
        const int v_ = (v);                                                                                                \
        const int64_t gx_ = ((P) / v_ + 255) / 256;                                                                        \
        const dim3 grid_((unsigned)gx_, reg_grid_y(gx_, N, 65536));                                                        \
        if (v_ == 8) hipLaunchKernelGGL((KERNEL<8, true>), grid_, dim3(256), 0, st, __VA_ARGS__);                          \
        else if (v_ == 4 && (dtype)) hipLaunchKernelGGL((KERNEL<4, true>), grid_, dim3(256), 0, st, __VA_ARGS__);          \
        else if (v_ == 4) hipLaunchKernelGGL((KERNEL<4, false>), grid_, dim3(256), 0, st, __VA_ARGS__);                    \
        else if (dtype) hipLaunchKernelGGL((KERNEL<1, true>), grid_, dim3(256), 0, st, __VA_ARGS__);                       \
        else hipLaunchKernelGGL((KERNEL<1, false>), grid_, dim3(256), 0, st, __VA_ARGS__);                                 \
    } while (0)

// ------------------------------------------------------------------------------------------------ the resampling of volumes
// What rshift3_kernel (register3d_ops.hip), rbwarp_kernel (register_blocks_ops.hip) and rrigid3_kernel (register_rigid_ops.hip) are
// made of.  out[n,z] = fl(w0 * p_0) + fl(w1 * p_1) with iz = floorf(dz), fz = fl(dz - iz), (w0, w1) = (fl(1 - fz), fz) and p_r the
// plane z + iz + r of volume n resampled in-plane by rshift_pixels (the bits of cwfa_reg_shift); a plane outside the volume holds
// `fill`; a plane of weight exactly 0 is neither read nor added (w0 == 0 happens: a tiny negative dz has fl(dz - iz) == 1); a
// non-finite component fills.
//
// A thread owns V consecutive voxels of a row and a segment of at most REG3_ZSEG planes, and walks z.  The segments of one (y, x) band
// have consecutive block indices, so they are in flight together and the plane two of them share is still in a cache.  The volumes
// are walked inside the kernels (blockIdx.y, + gridDim.y, ..).
#define REG_MAX_BLOCKS 4096           // blocks (nodes) of a grid: a volume's node table is then at most 48 KB
#define REG3_ZSEG 16

// what every entry point asks of a volume: sides that stay ints with a margin (z + iz + 1 with |iz| <= D + 1 stays an int, and so
// along y and x in rshift_pixels), fewer than 2^31 voxels
static inline bool reg3_sizes_ok(int D, int H, int W) {
    return D < (1 << 30) && H < (1 << 30) && W < (1 << 30) && (int64_t)D * H < ((int64_t)1 << 31) && (int64_t)D * H * W < ((int64_t)1 << 31);
}

// The checks the three resampling entry points share, in the order they make them (an entry point puts its own in between); `fn` is
// its name.  The windows' entry points make the one of the sizes too.  REG3_REQUIRE_STACK returns CWFA_OK for an empty stack.
#define REG3_REQUIRE_MODE(fn, mode) CWFA_REQUIRE((mode) == 0 || (mode) == 1, CWFA_E_INVAL, "%s: mode is 0 (bilinear) or 1 (nearest), got %d", fn, mode)
#define REG3_REQUIRE_SIZES(fn, N, D, H, W)                                                                                  \
    do {                                                                                                                   \
        CWFA_REQUIRE((N) >= 0 && (D) >= 0 && (H) >= 0 && (W) >= 0, CWFA_E_SHAPE, "%s: negative size", fn);                 \
        CWFA_REQUIRE(reg3_sizes_ok(D, H, W), CWFA_E_SHAPE, "%s: a volume of %d x %d x %d is too large", fn, D, H, W);      \
    } while (0)
#define REG3_REQUIRE_STACK(fn, in, out, N, D, H, W, vol_stride)                                                             \
    do {                                                                                                                   \
        CWFA_REQUIRE((out) != (in), CWFA_E_INVAL, "%s: out must not alias the stack", fn);                                 \
        if ((N) == 0 || (D) == 0 || (H) == 0 || (W) == 0) return CWFA_OK;                                                  \
        CWFA_REQUIRE((vol_stride) >= (int64_t)(D) * (H) * (W), CWFA_E_INVAL, "%s: volume stride smaller than a volume", fn); \
    } while (0)

// Launches KERNEL<V>(.., nseg, zseg, out): 16-byte stores where W and out's base allow (every row of every volume then starts on 16
// bytes; the loads take any alignment), even segments (96 planes are 6 x 16), ceil(H W / V / 256) * nseg <= D H W / 256 + D + nseg
// < 2^31 blocks along x by reg_grid_y blocks.
#define REG3_LAUNCH(KERNEL, N, D, H, W, out, st, ...)                                                                       \
    do {                                                                                                                   \
        const bool v4_ = ((W) & 3) == 0 && cwfa_aligned16(out);                                                            \
        const int nseg_ = ((D) + REG3_ZSEG - 1) / REG3_ZSEG, zseg_ = ((D) + nseg_ - 1) / nseg_;                            \
        const int64_t gx_ = ((((int64_t)(H) * (W) >> (v4_ ? 2 : 0)) + 255) / 256) * nseg_;                                 \
        const dim3 grid_((unsigned)gx_, reg_grid_y(gx_, N, 65536));                                                        \
        if (v4_) hipLaunchKernelGGL((KERNEL<4>), grid_, dim3(256), 0, st, __VA_ARGS__, nseg_, zseg_, out);                 \
        else hipLaunchKernelGGL((KERNEL<1>), grid_, dim3(256), 0, st, __VA_ARGS__, nseg_, zseg_, out);                     \
    } while (0)

// a thread's voxels (y, x0 .. x0 + V - 1), its offset p into a plane and its planes z0 .. z1 - 1; false for a thread past the plane
struct reg3_tile {
    int y, x0, z0, z1;
    int64_t p;
};
template <int V>
__device__ __forceinline__ bool reg3_tile_of(int D, int H, int W, int nseg, int zseg, reg3_tile& t) {
    const int Wv = W / V;                                             // V > 1: W is a multiple of V
    const int seg = (int)(blockIdx.x % (unsigned)nseg);
    const int64_t q = (int64_t)(blockIdx.x / (unsigned)nseg) * blockDim.x + threadIdx.x;
    if (q >= (int64_t)H * Wv) return false;
    t.y = (int)(q / Wv), t.x0 = (int)(q - (int64_t)t.y * Wv) * V;
    t.z0 = seg * zseg, t.z1 = t.z0 + zseg < D ? t.z0 + zseg : D;
    t.p = (int64_t)t.y * W + t.x0;
    return true;
}

// the split of a finite dz: plane offset iz (beyond +-(D + 1) every plane is outside whatever the value: clamped before the
// conversion to int) and the weights of planes z + iz and z + iz + 1; use0 and use1 are never both false: fz == 0 gives w0 == 1
struct reg3_zsplit {
    int iz;
    float w0, w1;
    bool use0, use1;
};
__device__ __forceinline__ reg3_zsplit reg3_zsplit_of(float dz, int nearest, int D) {
    if (nearest) dz = rintf(dz);                                      // rshift_pixels rounds (dy, dx) itself
    const float izf = floorf(dz);
    const float fz = __fsub_rn(dz, izf);
    reg3_zsplit s;
    s.iz = (int)fminf(fmaxf(izf, -(float)(D + 1)), (float)(D + 1));
    s.w0 = __fsub_rn(1.f, fz), s.w1 = fz;
    s.use0 = s.w0 != 0.f, s.use1 = s.w1 != 0.f;
    return s;
}
// the blend of the two resampled planes; the value of an unused one is not looked at
__device__ __forceinline__ float reg3_blend(const reg3_zsplit& s, float p0, float p1) {
    const float t0 = __fmul_rn(s.w0, p0), t1 = __fmul_rn(s.w1, p1);
    return s.use0 ? (s.use1 ? __fadd_rn(t0, t1) : t0) : t1;
}

// `fill` over a thread's segment: the volume's parameters are not finite.  o: the thread's voxels in plane 0 of the output volume
template <int V>
__device__ __forceinline__ void reg3_fill(float* __restrict__ o, int64_t HW, int z0, int z1, float fill) {
    typedef float fvec __attribute__((ext_vector_type(V)));
    fvec r;
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = fill;
    for (int z = z0; z < z1; ++z) *reinterpret_cast<fvec*>(o + (int64_t)z * HW) = r;
}

// The walk over z0 .. z1 - 1 for a displacement that does not change with z.  plane(zz, acc) resamples source plane zz, inside the
// volume, for the thread's V voxels; voxel j is `fill` where bad[j].  p_1 of plane z IS p_0 of plane z + 1 (the same function of the
// same source plane), so it is kept in registers and a source plane is read once per segment -- (ZSEG + 1) / ZSEG of the stack in
// all, whichever XCD's L2 a workgroup lands on.
template <int V, class Plane>
__device__ __forceinline__ void reg3_walk(float* __restrict__ o, int D, int64_t HW, int z0, int z1, const reg3_zsplit s, const bool (&bad)[V], float fill,
                                          Plane plane) {
    typedef float fvec __attribute__((ext_vector_type(V)));
    auto at = [&](int zz, float(&acc)[V]) {
        if (zz < 0 || zz >= D) {
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = fill;
        } else {
            plane(zz, acc);
        }
    };
    float a[V] = {}, b[V] = {};                                       // the unused one of the two stays 0 and is not read
    if (s.use0) at(z0 + s.iz, a);
    for (int z = z0; z < z1; ++z) {
        if (s.use1) at(z + s.iz + 1, b);
        fvec r;
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = bad[j] ? fill : reg3_blend(s, a[j], b[j]);
        *reinterpret_cast<fvec*>(o + (int64_t)z * HW) = r;
        if (s.use0 && s.use1) {                                       // plane z + iz + 1 is the next step's first plane
#pragma unroll
            for (int j = 0; j < V; ++j) a[j] = b[j];
        } else if (s.use0 && z + 1 < z1) {
            at(z + 1 + s.iz, a);
        }
    }
}
