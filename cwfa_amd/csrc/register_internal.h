// What the resampling kernels of the registration share (register_ops.hip: one shift per frame; register_views_ops.hip: one shift
// per pixel label): the arithmetic of step 7 of DESIGN.md section 26.1 for V consecutive pixels of a row, and the grid rule of the
// kernels whose threads walk the frames.  One definition, so that the labelled form is the rigid form's bits by construction.
#pragma once
#include <math.h>
#include <type_traits>
#include "common.h"

// blocks along y for a kernel whose threads walk the frames: about `target` blocks in all, the per-pixel values reused over N / gy
// frames.  The window and the resampling keep a few words per thread and take many blocks (an even tail); the whitening keeps a
// plane of weights and takes one block row where the bins alone fill the chip, so that the plane is read once.
static inline unsigned reg_grid_y(int64_t gx, int N, int64_t target) {
    int64_t gy = target / gx < 1 ? 1 : target / gx;
    gy = gy > 65535 ? 65535 : gy;
    return (unsigned)(gy > N ? N : gy);
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
