// Small HBM-bound kernels of the LRNN (UNet + ConvNeXt + GlobalAttention): normalisation statistics and applies,
// adaptive max-pool, attention/combine.  The convolutions themselves are in conv2d.hip.
#include "common.h"

// ------------------------------------------------------------------------------------------------ BatchNorm statistics
// grid (splits, C, B): each block sums a contiguous slice of one (sample, channel) plane and adds (sum, sumsq) in double.
// Per thread the partial sums of <= 64 elements stay in fp32 pairs feeding doubles (the products are exact in double).
__global__ __launch_bounds__(256) void channel_stats_kernel(const float* __restrict__ x, double* __restrict__ stats, int64_t HW,
                                                            int64_t x_bs, int vec_ok) {
    __shared__ double red[16];
    const int c = blockIdx.y;
    const float* p = x + (int64_t)blockIdx.z * x_bs + (int64_t)c * HW;
    const int64_t per = (((HW + gridDim.x - 1) / gridDim.x) + 3) & ~(int64_t)3;      // slices start on 16-byte boundaries
    const int64_t lo = (int64_t)blockIdx.x * per < HW ? (int64_t)blockIdx.x * per : HW, hi = lo + per < HW ? lo + per : HW;
    double s = 0.0, q = 0.0;
    if (vec_ok && (lo & 3) == 0) {
        const int64_t n4 = (hi - lo) >> 2;
        const f32x4* p4 = reinterpret_cast<const f32x4*>(p + lo);
        int64_t i = threadIdx.x;
        for (; i + 3 * (int64_t)blockDim.x < n4; i += 4 * (int64_t)blockDim.x) {        // four 16-byte loads in flight per thread
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = p4[i + u * (int64_t)blockDim.x];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s += ((double)v[u][0] + (double)v[u][1]) + ((double)v[u][2] + (double)v[u][3]);
                q += ((double)v[u][0] * v[u][0] + (double)v[u][1] * v[u][1]) + ((double)v[u][2] * v[u][2] + (double)v[u][3] * v[u][3]);
            }
        }
        for (; i < n4; i += blockDim.x) {
            const f32x4 v = p4[i];
            s += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
            q += ((double)v[0] * v[0] + (double)v[1] * v[1]) + ((double)v[2] * v[2] + (double)v[3] * v[3]);
        }
        for (int64_t i = lo + (n4 << 2) + threadIdx.x; i < hi; i += blockDim.x) {
            const float v = p[i];
            s += v;
            q += (double)v * v;
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            const float v = p[i];
            s += v;
            q += (double)v * v;
        }
    }
    s = cwfa_block_sum(s, red);
    q = cwfa_block_sum(q, red);
    if (threadIdx.x == 0) {
        atomicAdd(&stats[2 * c], s);
        atomicAdd(&stats[2 * c + 1], q);
    }
}

extern "C" int cwfa_channel_stats_f32(const float* x, double* stats, int B, int C, int64_t HW, int64_t x_bs, void* stream) {
    CWFA_REQUIRE(x && stats, CWFA_E_INVAL, "cwfa_channel_stats_f32: null pointer");
    CWFA_REQUIRE(B >= 0 && C >= 0 && HW >= 0 && C <= 65535 && B <= 65535, CWFA_E_SHAPE, "cwfa_channel_stats_f32: bad shape");
    if (B == 0 || C == 0 || HW == 0) return CWFA_OK;
    // enough blocks to fill the chip several times over (256 CUs x 8 resident blocks), but as few atomics and as long
    // streams per block as that allows: ~4096 blocks in all, >= 16 elements per thread
    int splits = (int)((HW + 256 * 16 - 1) / (256 * 16));
    const int64_t want = (4096 + (int64_t)C * B - 1) / ((int64_t)C * B);
    if (splits > want) splits = (int)want;
    if (splits < 1) splits = 1;
    if (splits > 64) splits = 64;
    const int vec_ok = (HW & 3) == 0 && (x_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    hipLaunchKernelGGL(channel_stats_kernel, dim3(splits, C, B), dim3(256), 0, (hipStream_t)stream, x, stats, HW, x_bs, vec_ok);
    CWFA_LAUNCH_CHECK("cwfa_channel_stats_f32");
    return CWFA_OK;
}


__global__ void bn_fold_kernel(const double* __restrict__ stats, double count, const float* __restrict__ rm,
                               const float* __restrict__ rv, const float* __restrict__ w, const float* __restrict__ bsh,
                               float eps, const float* __restrict__ mask, int B, float* __restrict__ scale,
                               float* __restrict__ shift, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double sc = 1.0, sh = 0.0;
    if (stats || rm) {
        double mean, var;
        if (stats) {
            mean = stats[2 * c] / count;
            var = stats[2 * c + 1] / count - mean * mean;
            if (var < 0.0) var = 0.0;
        } else {
            mean = rm[c];
            var = rv[c];
        }
        sc = (w ? (double)w[c] : 1.0) / sqrt(var + (double)eps);
        sh = (bsh ? (double)bsh[c] : 0.0) - mean * sc;
    }
    if (mask) {
        for (int b = 0; b < B; ++b) {
            const float m = mask[b * C + c];
            scale[b * C + c] = (float)sc * m;
            shift[b * C + c] = (float)sh * m;
        }
    } else {
        scale[c] = (float)sc;
        shift[c] = (float)sh;
    }
}

// Everything that follows the statistics pass of a train-mode BatchNorm2d in ONE launch (the inference path issued a fill, the
// fold, the running-buffer update and three elementwise kernels for the dropout mask per layer -- ~40 tiny launches per volume):
// (scale, shift) as bn_fold_kernel; running_mean / running_var / num_batches_tracked as bn_running_update_kernel; the dropout
// factor from the raw uniform draw, m = (u >= p) / (1 - p) (F.dropout2d, unet.py:80,86); and the statistics buffer is zeroed
// for its next use.
__global__ void bn_finish_kernel(double* __restrict__ stats, double count, float* __restrict__ rm, float* __restrict__ rv,
                                 long long* __restrict__ nbt, float momentum, int update_running, const float* __restrict__ w,
                                 const float* __restrict__ bsh, float eps, const float* __restrict__ mask,
                                 const float* __restrict__ mask_u, float drop_p, float keep_scale, int B, float* __restrict__ scale,
                                 float* __restrict__ shift, int C, int zero_stats) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && nbt && update_running) *nbt += 1;
    if (c >= C) return;
    double sc = 1.0, sh = 0.0;
    if (stats || rm) {
        double mean, var;
        if (stats) {
            const double s1 = stats[2 * c], s2 = stats[2 * c + 1];
            mean = s1 / count;
            var = s2 / count - mean * mean;
            if (var < 0.0) var = 0.0;
            if (update_running) {
                const double var_u = (s2 - s1 * mean) / (count > 1.0 ? count - 1.0 : 1.0);
                rm[c] = rm[c] * (1.f - momentum) + momentum * (float)mean;
                rv[c] = rv[c] * (1.f - momentum) + momentum * (float)var_u;
            }
            if (zero_stats) stats[2 * c] = stats[2 * c + 1] = 0.0;
        } else {
            mean = rm[c];
            var = rv[c];
        }
        sc = (w ? (double)w[c] : 1.0) / sqrt(var + (double)eps);
        sh = (bsh ? (double)bsh[c] : 0.0) - mean * sc;
    }
    if (mask || mask_u) {
        for (int b = 0; b < B; ++b) {
            const float m = mask ? mask[b * C + c] : (mask_u[b * C + c] >= drop_p ? 1.f : 0.f) / keep_scale;
            scale[b * C + c] = (float)sc * m;
            shift[b * C + c] = (float)sh * m;
        }
    } else {
        scale[c] = (float)sc;
        shift[c] = (float)sh;
    }
}

extern "C" int cwfa_bn_finish_f32(double* stats, double count, float* running_mean, float* running_var, long long* num_batches_tracked,
                                  float momentum, int update_running, const float* weight, const float* bias, float eps,
                                  const float* mask_bc, const float* mask_u, float drop_p, float keep_scale, int B, float* scale,
                                  float* shift, int C, int zero_stats, void* stream) {
    CWFA_REQUIRE(scale && shift, CWFA_E_INVAL, "cwfa_bn_finish_f32: null output");
    CWFA_REQUIRE(stats || (running_mean && running_var) || mask_bc || mask_u, CWFA_E_INVAL,
                 "cwfa_bn_finish_f32: neither batch nor running statistics nor a mask");
    CWFA_REQUIRE(!running_mean == !running_var, CWFA_E_INVAL, "cwfa_bn_finish_f32: running_mean and running_var go together");
    CWFA_REQUIRE(!(mask_bc && mask_u), CWFA_E_INVAL, "cwfa_bn_finish_f32: a mask OR a uniform draw");
    CWFA_REQUIRE(!(mask_bc || mask_u) || B > 0, CWFA_E_INVAL, "cwfa_bn_finish_f32: mask needs B > 0");
    CWFA_REQUIRE(!mask_u || (drop_p >= 0.f && drop_p < 1.f), CWFA_E_INVAL, "cwfa_bn_finish_f32: 0 <= drop_p < 1");
    CWFA_REQUIRE(!stats || count > 0, CWFA_E_INVAL, "cwfa_bn_finish_f32: count must be positive");
    CWFA_REQUIRE(!update_running || (stats && running_mean), CWFA_E_INVAL, "cwfa_bn_finish_f32: the running update needs statistics and buffers");
    CWFA_REQUIRE(C >= 0, CWFA_E_INVAL, "cwfa_bn_finish_f32: negative size");
    if (C == 0) return CWFA_OK;
    CWFA_REQUIRE(!mask_u || keep_scale > 0.f, CWFA_E_INVAL, "cwfa_bn_finish_f32: keep_scale = fp32(1 - p) must be positive");
    hipLaunchKernelGGL(bn_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, stats, count, running_mean, running_var,
                       num_batches_tracked, momentum, update_running, weight, bias, eps, mask_bc, mask_u, drop_p, keep_scale, B, scale,
                       shift, C, zero_stats);
    CWFA_LAUNCH_CHECK("cwfa_bn_finish_f32");
    return CWFA_OK;
}

// nn.BatchNorm2d's train-mode buffer bookkeeping in one launch (torch/nn/modules/batchnorm.py via unet.py:101-107):
// running_mean <- (1-m) running_mean + m mean,  running_var <- (1-m) running_var + m var_unbiased,  num_batches_tracked += 1
__global__ void bn_running_update_kernel(const double* __restrict__ stats, double count, float momentum, float* __restrict__ rm,
                                         float* __restrict__ rv, long long* __restrict__ nbt, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && nbt) *nbt += 1;
    if (c >= C) return;
    const double mean = stats[2 * c] / count;
    const double var_u = (stats[2 * c + 1] - stats[2 * c] * mean) / (count > 1.0 ? count - 1.0 : 1.0);
    rm[c] = rm[c] * (1.f - momentum) + momentum * (float)mean;
    rv[c] = rv[c] * (1.f - momentum) + momentum * (float)var_u;
}

extern "C" int cwfa_bn_running_update_f32(const double* stats, double count, float momentum, float* running_mean,
                                          float* running_var, long long* num_batches_tracked, int C, void* stream) {
    CWFA_REQUIRE(stats && running_mean && running_var, CWFA_E_INVAL, "cwfa_bn_running_update_f32: null pointer");
    CWFA_REQUIRE(C >= 0 && count > 0.0, CWFA_E_INVAL, "cwfa_bn_running_update_f32: bad size");
    if (C == 0) return CWFA_OK;
    hipLaunchKernelGGL(bn_running_update_kernel, dim3((C + 127) / 128), dim3(128), 0, (hipStream_t)stream, stats, count, momentum,
                       running_mean, running_var, num_batches_tracked, C);
    CWFA_LAUNCH_CHECK("cwfa_bn_running_update_f32");
    return CWFA_OK;
}

extern "C" int cwfa_bn_fold_f32(const double* stats, double count, const float* running_mean, const float* running_var,
                                const float* weight, const float* bias, float eps, const float* mask_bc, int B, float* scale,
                                float* shift, int C, void* stream) {
    CWFA_REQUIRE(scale && shift, CWFA_E_INVAL, "cwfa_bn_fold_f32: null output");
    CWFA_REQUIRE(stats || (running_mean && running_var) || mask_bc, CWFA_E_INVAL,
                 "cwfa_bn_fold_f32: neither batch nor running statistics nor a mask");
    CWFA_REQUIRE(!running_mean == !running_var, CWFA_E_INVAL, "cwfa_bn_fold_f32: running_mean and running_var go together");
    CWFA_REQUIRE(!mask_bc || B > 0, CWFA_E_INVAL, "cwfa_bn_fold_f32: mask needs B > 0");
    CWFA_REQUIRE(!stats || count > 0, CWFA_E_INVAL, "cwfa_bn_fold_f32: count must be positive");
    CWFA_REQUIRE(C >= 0, CWFA_E_INVAL, "cwfa_bn_fold_f32: negative size");
    if (C == 0) return CWFA_OK;
    hipLaunchKernelGGL(bn_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, stats, count, running_mean,
                       running_var, weight, bias, eps, mask_bc, B, scale, shift, C);
    CWFA_LAUNCH_CHECK("cwfa_bn_fold_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ adaptive max pool
// window of output i along a dimension of size n -> m:  [floor(i*n/m), ceil((i+1)*n/m))   (ATen adaptive pooling)
__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                      float* __restrict__ full, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, int C, int H, int W, int Ho, int Wo) {
    const int64_t n = (int64_t)Ho * Wo;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int bc = blockIdx.y, c = bc % C;
    const int oy = (int)(i / Wo), ox = (int)(i % Wo);
    const int y0 = (int)(((int64_t)oy * H) / Ho), y1 = (int)((((int64_t)oy + 1) * H + Ho - 1) / Ho);
    const int x0 = (int)(((int64_t)ox * W) / Wo), x1 = (int)((((int64_t)ox + 1) * W + Wo - 1) / Wo);
    const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
    const float* px = x + (int64_t)bc * H * W;
    float* pf = full ? full + (int64_t)bc * H * W : nullptr;
    float m = -INFINITY;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
            float v = px[(int64_t)yy * W + xx];
            if (scale) v = v * sc + sh;
            // overlapping adaptive windows (H % Ho != 0) rewrite the same value: benign
            if (pf) pf[(int64_t)yy * W + xx] = v;
            m = (v > m || v != v) ? v : m;      // NaN propagates like ATen
        }
    y[(int64_t)bc * n + i] = m;
}

// exact 2x2 windows (H = 2 Ho, W = 2 Wo, W % 4 == 0, 16-byte aligned rows): a thread owns two output pixels = 4 x 2 inputs,
// 16-byte loads / stores (the UNet's pooling, unet.py:79, always has this shape)
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ full,
                                                         const float* __restrict__ scale, const float* __restrict__ shift, int C,
                                                         int H, int W) {
    const int Wo = W >> 1, Ho = H >> 1, wq = W >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)Ho * wq) return;
    const int bc = blockIdx.y, c = bc % C;
    const int oy = (int)(i / wq), q = (int)(i % wq);
    const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
    const int64_t o = (int64_t)bc * H * W + (int64_t)(2 * oy) * W + 4 * q;
    f32x4 r0 = *reinterpret_cast<const f32x4*>(x + o), r1 = *reinterpret_cast<const f32x4*>(x + o + W);
    if (scale) {
        r0 = r0 * sc + sh;
        r1 = r1 * sc + sh;
    }
    if (full) {
        *reinterpret_cast<f32x4*>(full + o) = r0;
        *reinterpret_cast<f32x4*>(full + o + W) = r1;
    }
    float m[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {               // same visiting order as the generic kernel: (0,0) (0,1) (1,0) (1,1); NaN propagates
        float a = -INFINITY;
        const float v4[4] = {r0[2 * k], r0[2 * k + 1], r1[2 * k], r1[2 * k + 1]};
#pragma unroll
        for (int j = 0; j < 4; ++j) a = (v4[j] > a || v4[j] != v4[j]) ? v4[j] : a;
        m[k] = a;
    }
    *reinterpret_cast<float2*>(y + (int64_t)bc * Ho * Wo + (int64_t)oy * Wo + 2 * q) = make_float2(m[0], m[1]);
}

extern "C" int cwfa_maxpool_f32(const float* x, float* y, float* full, const float* scale, const float* shift, int B, int C,
                                int H, int W, int Ho, int Wo, void* stream) {
    CWFA_REQUIRE(x && y, CWFA_E_INVAL, "cwfa_maxpool_f32: null pointer");
    CWFA_REQUIRE(!(scale && !shift), CWFA_E_INVAL, "cwfa_maxpool_f32: scale without shift");
    CWFA_REQUIRE(B >= 0 && C >= 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && Ho <= H && Wo <= W, CWFA_E_SHAPE,
                 "cwfa_maxpool_f32: bad shape");
    CWFA_REQUIRE((int64_t)B * C <= 65535, CWFA_E_SHAPE, "cwfa_maxpool_f32: B*C too large");
    if (B == 0 || C == 0) return CWFA_OK;
    const int64_t n = (int64_t)Ho * Wo;
    if (H == 2 * Ho && W == 2 * Wo && (W & 3) == 0 && cwfa_aligned16(x) && (!full || cwfa_aligned16(full)) &&
        (reinterpret_cast<uintptr_t>(y) & 7) == 0) {
        hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)((n / 2 + 255) / 256), B * C), dim3(256), 0, (hipStream_t)stream, x, y, full,
                           scale, shift, C, H, W);
        CWFA_LAUNCH_CHECK("cwfa_maxpool_f32");
        return CWFA_OK;
    }
    hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)((n + 255) / 256), B * C), dim3(256), 0, (hipStream_t)stream, x, y, full,
                       scale, shift, C, H, W, Ho, Wo);
    CWFA_LAUNCH_CHECK("cwfa_maxpool_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ LayerNorm over (C,H,W)
__global__ __launch_bounds__(256) void sample_stats_kernel(const float* __restrict__ x, double* __restrict__ stats,
                                                           int64_t CHW) {
    __shared__ double red[16];
    const int b = blockIdx.y;
    const float* px = x + (int64_t)b * CHW;
    double s = 0.0, q = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < CHW; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = px[i];
        s += v;
        q += (double)v * v;
    }
    s = cwfa_block_sum(s, red);
    q = cwfa_block_sum(q, red);
    if (threadIdx.x == 0) {
        atomicAdd(&stats[2 * b], s);
        atomicAdd(&stats[2 * b + 1], q);
    }
}

extern "C" int cwfa_sample_stats_f32(const float* x, double* stats, int B, int64_t CHW, void* stream) {
    CWFA_REQUIRE(x && stats, CWFA_E_INVAL, "cwfa_sample_stats_f32: null pointer");
    CWFA_REQUIRE(B >= 0 && CHW >= 0 && B <= 65535, CWFA_E_SHAPE, "cwfa_sample_stats_f32: bad shape");
    if (B == 0 || CHW == 0) return CWFA_OK;
    int blocks = (int)((CHW + 256 * 16 - 1) / (256 * 16));
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(sample_stats_kernel, dim3(blocks, B), dim3(256), 0, (hipStream_t)stream, x, stats, CHW);
    CWFA_LAUNCH_CHECK("cwfa_sample_stats_f32");
    return CWFA_OK;
}

// The LayerNorm expression, shared by the apply kernel and the fused ConvNeXt tail (convnext_tail_kernel) so that both form the
// same bits: mean and rstd of sample b from its float64 (sum, sum of squares), the mean rounded to fp32, rstd from a float64 sqrt
__device__ __forceinline__ void cwfa_ln_coefs(const double* __restrict__ stats, int b, int64_t CHW, float eps, float& mean_f, float& rstd) {
    const double mean = stats[2 * b] / (double)CHW;
    double var = stats[2 * b + 1] / (double)CHW - mean * mean;
    if (var < 0.0) var = 0.0;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
    mean_f = (float)mean;
}
__device__ __forceinline__ float cwfa_ln_apply(float x, float mean, float rstd, float w, float b) {
    const float v = (x - mean) * rstd;
    return v * w + b;
}

__global__ __launch_bounds__(256) void layernorm_apply_kernel(const float* __restrict__ x, const double* __restrict__ stats,
                                                              const float* __restrict__ w, const float* __restrict__ bsh,
                                                              float eps, float* __restrict__ y, int64_t CHW) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= CHW) return;
    const int b = blockIdx.y;
    float mean, rstd;
    cwfa_ln_coefs(stats, b, CHW, eps, mean, rstd);
    y[(int64_t)b * CHW + i] = cwfa_ln_apply(x[(int64_t)b * CHW + i], mean, rstd, w ? w[i] : 1.f, bsh ? bsh[i] : 0.f);
}

extern "C" int cwfa_layernorm_apply_f32(const float* x, const double* stats, const float* w, const float* b, float eps,
                                        float* y, int B, int64_t CHW, void* stream) {
    CWFA_REQUIRE(x && stats && y, CWFA_E_INVAL, "cwfa_layernorm_apply_f32: null pointer");
    CWFA_REQUIRE(B >= 0 && CHW >= 0 && B <= 65535, CWFA_E_SHAPE, "cwfa_layernorm_apply_f32: bad shape");
    if (B == 0 || CHW == 0) return CWFA_OK;
    hipLaunchKernelGGL(layernorm_apply_kernel, dim3((unsigned)((CHW + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, x,
                       stats, w, b, eps, y, CHW);
    CWFA_LAUNCH_CHECK("cwfa_layernorm_apply_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ the ConvNeXt block's tail
// y[b,co,p] = GELU(b1[co] + sum_ci W1[co,ci] LN(v)[b,ci,p]) + gate[b] u[b,co,p]        (networks.py:490-503; C <= 64)
// in ONE pass: LayerNorm apply, the 1x1, GELU, the drop-path gate and the residual -- what layernorm_apply, scale_channels and the
// fp32 1x1 launch did with three more trips of the map through memory.  fp32 on v_mfma_f32_32x32x2_f32, k ascending from a zero
// accumulator: the fmaf chain of conv2d_mfma_kernel, so the result is that sequence's bit for bit.
//   M = output channels (MT = 1 or 2 tiles of 32), N = 32 consecutive pixels of the flattened plane, K = channel pairs.
//   B operand: lane (k = lane >> 5, pixel = lane & 31) loads v, the LayerNorm weight and bias of its (channel, pixel) from global
//   memory -- 128 contiguous bytes per half-wave and channel -- and normalises in registers: no LDS staging, no barrier in the loop.
//   Channels >= C and pixels >= HW are out of range of the buffer descriptors (0.0, never read); K is padded to whole chunks of 16
//   channels with zero weights.
//   A operand: W1 in torch layout [co][ci], copied once per block into LDS rows of KP + 1 floats (odd stride: the 32 rows of a
//   fragment read fall on different banks), zero beyond C.  A block (four waves) walks pixel tiles blockIdx.x * 4 + wave + k * grid.
//   Loads run one chunk (8 k-steps: 24 values per lane) ahead of the MFMAs; a tile's first chunk is requested in front of the
//   epilogue of the tile before it (the first one in front of the LDS fill), so a wave always has loads in flight.
//   Residual: u from memory, or (XRES, c_in <= 8) formed here as the fp32 1x1 kernel forms it: fmaf over ci ascending from 0.0f,
//   then + b0.  gate * u is a rounded product and the sum a rounded sum (scale_channels stored the product).
struct TailParams {
    const float *v, *lw, *lb, *w1, *b1, *u, *gate, *x, *w0, *b0;
    const double* stats;
    float* y;
    float eps;
    int C, c_in, KP;
    int64_t HW, v_bs, u_bs, x_bs, y_bs, ntiles;
};

template <int MT, bool XRES>
__global__ __launch_bounds__(256, 4) void convnext_tail_kernel(TailParams p) {
    constexpr int KC = 8;                                     // k-steps per chunk
    constexpr unsigned OOB = 0x80000000u;
    __shared__ float Ws[MT * 32 * 65];
    __shared__ float Es[MT * 32 * 10];                        // per output channel: W0[co][0..7], b0[co], b1[co]
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, C = p.C, LS = p.KP + 1;
    const int plane = (int)(p.HW * 4);
    const int cbytes = C * plane;
    const auto rv = CWFA_RSRC(p.v + (int64_t)b * p.v_bs, cbytes);
    const auto rlw = CWFA_RSRC(p.lw, cbytes);
    const auto rlb = CWFA_RSRC(p.lb, cbytes);
    const auto ru = CWFA_RSRC(XRES ? p.v : p.u + (int64_t)b * p.u_bs, XRES ? 0 : cbytes);
    const auto rx = CWFA_RSRC(XRES ? p.x + (int64_t)b * p.x_bs : p.v, XRES ? p.c_in * plane : 0);
    const auto ry = CWFA_RSRC(p.y + (int64_t)b * p.y_bs, cbytes);
    auto ldf = [](decltype(rv) r, unsigned vo, int so) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0)); };
    // (32-bit indices: the entry point holds (C + 23) * HW * 4 below 2^31)
    const int HW = (int)p.HW, ntiles = (int)p.ntiles, tstep = (int)gridDim.x * 4;
    float xa[KC], wa[KC], ba[KC], xb[KC], wb[KC], bb[KC];
    // B operand offset of a tile: channel 2 kk + kh of pixel tile * 32 + l31 (out of range beyond the plane)
    auto vo_of = [&](int tile) { const int px = tile * 32 + l31; return px < HW ? (unsigned)(px + kh * HW) * 4u : OOB; };
    auto load = [&](float (&xv)[KC], float (&wv)[KC], float (&bv)[KC], unsigned vo, int c) {
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int so = (c * KC + j) * 2 * plane;
            xv[j] = ldf(rv, vo, so);
            wv[j] = ldf(rlw, vo, so);
            bv[j] = ldf(rlb, vo, so);
        }
    };
    // the first tile's first chunk is requested before the weights are staged: the fill and its barrier run under those loads
    int tile = (int)blockIdx.x * 4 + wave;
    unsigned vo = vo_of(tile);
    if (tile < ntiles) load(xa, wa, ba, vo, 0);
    CWFA_FENCE();

    for (int co = tid >> 6, ci = tid & 63; co < MT * 32; co += 4)      // a wave per row: 256 contiguous bytes of W1, no division
        if (ci < p.KP) Ws[co * LS + ci] = (co < C && ci < C) ? p.w1[co * C + ci] : 0.f;
    for (int e = tid; e < MT * 32 * 10; e += 256) {
        const int co = e / 10, j = e % 10;
        float val = 0.f;
        if (co < C) {
            if (j < 8) val = (XRES && j < p.c_in) ? p.w0[co * p.c_in + j] : 0.f;
            else if (j == 8) val = (XRES && p.b0) ? p.b0[co] : 0.f;
            else val = p.b1 ? p.b1[co] : 0.f;
        }
        Es[e] = val;
    }
    __syncthreads();

    float mean, rstd;
    cwfa_ln_coefs(p.stats, b, (int64_t)C * p.HW, p.eps, mean, rstd);
    const float gate = p.gate ? p.gate[b] : 1.f;
    const bool gated = p.gate != nullptr;
    const float* wl = Ws + l31 * LS + kh;
    const float* el = Es + 4 * kh * 10;                       // this lane half's rows of Es
    const int nch = p.KP / (2 * KC);
    auto run = [&](f32x16 (&acc)[MT], const float (&xv)[KC], const float (&wv)[KC], const float (&bv)[KC], int c) {
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const float bq = cwfa_ln_apply(xv[j], mean, rstd, wv[j], bv[j]);
#pragma unroll
            for (int m = 0; m < MT; ++m)
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(wl[m * 32 * LS + (c * KC + j) * 2], bq, acc[m], 0, 0, 0);
        }
    };

    while (tile < ntiles) {                                   // (wave-uniform) chunk 0 of this tile is in flight in xa / wa / ba
        const int px = tile * 32 + l31;
        const bool ok = px < HW;
        f32x16 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
#pragma unroll 1
        for (int c = 0; c < nch; c += 2) {
            if (c + 1 < nch) load(xb, wb, bb, vo, c + 1);
            CWFA_FENCE();
            run(acc, xa, wa, ba, c);
            CWFA_FENCE();
            if (c + 1 < nch) {
                if (c + 2 < nch) load(xa, wa, ba, vo, c + 2);
                CWFA_FENCE();
                run(acc, xb, wb, bb, c + 1);
                CWFA_FENCE();
            }
        }

        // ---- epilogue: register r of tile m = channel m*32 + row(r, kh) of pixel px; rows >= C are out of the descriptors' range
        const unsigned eo = ok ? (unsigned)(px + 4 * kh * HW) * 4u : OOB;
        float xin[8];
        if constexpr (XRES) {
            const unsigned pb = ok ? (unsigned)px * 4u : OOB;                               // this lane's pixel, channel 0
#pragma unroll
            for (int ci = 0; ci < 8; ++ci) xin[ci] = ldf(rx, pb, ci * plane);
        }
        // the next tile's first chunk goes out in front of the epilogue's vector work (xa / wa / ba are free: the chunk loop has consumed them)
        tile += tstep;
        vo = vo_of(tile);
        if (tile < ntiles) load(xa, wa, ba, vo, 0);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float uu[XRES ? 1 : 16];
            if constexpr (!XRES) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (m * 32 + cwfa_acc_row(r, 0) < C) uu[r] = ldf(ru, eo, (m * 32 + cwfa_acc_row(r, 0)) * plane);
            }
            CWFA_FENCE();
            // (fenced per element: unfenced, hipcc hoists the LDS reads and erf polynomials of all 16 and spills)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c0 = m * 32 + cwfa_acc_row(r, 0);
                if (c0 >= C) continue;                     // (uniform) rows of both lane halves past the last channel: no GELU for nothing
                float ur;
                if constexpr (XRES) {
                    float a = 0.0f;
#pragma unroll
                    for (int ci = 0; ci < 8; ++ci) a = fmaf(el[c0 * 10 + ci], xin[ci], a);
                    ur = a + el[c0 * 10 + 8];
                } else {
                    ur = uu[r];
                }
                const float t = cwfa_gelu(acc[m][r] + el[c0 * 10 + 9]);
                const float res = gated ? __fmul_rn(ur, gate) : ur;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, __fadd_rn(t, res)), ry, eo, c0 * plane, 0);
                CWFA_FENCE();
            }
        }
    }
}

extern "C" int cwfa_convnext_tail_f32(const float* v, const double* stats, const float* lw, const float* lb, float eps,
                                      const float* w1, const float* b1, const float* u, const float* gate, const float* x,
                                      const float* w0, const float* b0, int c_in, float* y, int B, int C, int64_t HW,
                                      int64_t v_bs, int64_t u_bs, int64_t x_bs, int64_t y_bs, void* stream) {
    CWFA_REQUIRE(B >= 0 && B <= 65535 && C > 0 && C <= 64 && HW >= 0, CWFA_E_SHAPE, "cwfa_convnext_tail_f32: bad shape (C <= 64)");
    if (B == 0 || HW == 0) return CWFA_OK;
    CWFA_REQUIRE(v && stats && lw && lb && w1 && y, CWFA_E_INVAL, "cwfa_convnext_tail_f32: null pointer");
    CWFA_REQUIRE((u != nullptr) != (x != nullptr), CWFA_E_INVAL, "cwfa_convnext_tail_f32: exactly one of u (the residual) and x (the block input it is formed from)");
    CWFA_REQUIRE(!x || (w0 && c_in > 0 && c_in <= 8), CWFA_E_INVAL, "cwfa_convnext_tail_f32: the residual is formed from at most 8 input channels and needs w0");
    CWFA_REQUIRE((int64_t)(C + 15 + 8) * HW * 4 < (1ll << 31), CWFA_E_SHAPE, "cwfa_convnext_tail_f32: one sample's map must stay below 2 GiB (32-bit buffer offsets)");
    TailParams p{};
    p.v = v; p.lw = lw; p.lb = lb; p.w1 = w1; p.b1 = b1; p.u = u; p.gate = gate; p.x = x; p.w0 = w0; p.b0 = b0;
    p.stats = stats; p.y = y; p.eps = eps; p.C = C; p.c_in = c_in; p.KP = (C + 15) / 16 * 16;
    p.HW = HW; p.v_bs = v_bs; p.u_bs = u_bs; p.x_bs = x_bs; p.y_bs = y_bs;
    p.ntiles = (HW + 31) / 32;
    // four blocks of four waves per CU over the chip; at least one tile per wave
    int64_t gx = (p.ntiles + 3) / 4;
    const int64_t cap = B >= 1024 ? 1 : 1024 / B;
    if (gx > cap) gx = cap;
    const dim3 grid((unsigned)gx, B);
    hipStream_t st = (hipStream_t)stream;
    if (C <= 32) {
        if (x) hipLaunchKernelGGL((convnext_tail_kernel<1, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((convnext_tail_kernel<1, false>), grid, dim3(256), 0, st, p);
    } else {
        if (x) hipLaunchKernelGGL((convnext_tail_kernel<2, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((convnext_tail_kernel<2, false>), grid, dim3(256), 0, st, p);
    }
    CWFA_LAUNCH_CHECK("cwfa_convnext_tail_f32");
    return CWFA_OK;
}

// ------------------------------------------------------------------------------------------------ attention + combine
#define CWFA_ATT_MAXC 16
__global__ __launch_bounds__(256) void attention_combine_kernel(const float* __restrict__ mean, const float* __restrict__ w1,
                                                                const float* __restrict__ b1, const float* __restrict__ w2,
                                                                const float* __restrict__ b2, const float* __restrict__ m,
                                                                const float* __restrict__ x, float* __restrict__ out, int C,
                                                                int64_t L) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const int b = blockIdx.y;
    const float* pm = mean + (int64_t)b * C * L;
    float hid[CWFA_ATT_MAXC];
    for (int o = 0; o < C; ++o) hid[o] = b1[o];
    for (int c = 0; c < C; ++c) {
        const float vm = i > 0 ? pm[(int64_t)c * L + i - 1] : 0.f;
        const float v0 = pm[(int64_t)c * L + i];
        const float vp = i + 1 < L ? pm[(int64_t)c * L + i + 1] : 0.f;
        for (int o = 0; o < C; ++o) {
            const float* ww = w1 + ((int64_t)o * C + c) * 3;
            hid[o] = fmaf(ww[2], vp, fmaf(ww[1], v0, fmaf(ww[0], vm, hid[o])));
        }
    }
    for (int o = 0; o < C; ++o) hid[o] = hid[o] > 0.f ? hid[o] : 0.f;
    for (int o = 0; o < C; ++o) {
        float a = b2[o];
        for (int c = 0; c < C; ++c) a = fmaf(w2[o * C + c], hid[c], a);
        const float att = 1.f / (1.f + expf(-a));
        const int64_t idx = ((int64_t)b * C + o) * L + i;
        out[idx] = m ? (x ? x[idx] : 0.f) + (m[idx] * 2.f) * (att - 0.5f) : att;
    }
}

extern "C" int cwfa_attention_combine_f32(const float* mean, const float* w1, const float* b1, const float* w2,
                                          const float* b2, const float* m, const float* x, float* out, int B, int C,
                                          int64_t HW, void* stream) {
    CWFA_REQUIRE(mean && w1 && b1 && w2 && b2 && out, CWFA_E_INVAL, "cwfa_attention_combine_f32: null pointer");
    CWFA_REQUIRE(C > 0 && C <= CWFA_ATT_MAXC, CWFA_E_SHAPE, "cwfa_attention_combine_f32: C=%d not in 1..%d", C, CWFA_ATT_MAXC);
    CWFA_REQUIRE(B >= 0 && HW >= 0 && B <= 65535, CWFA_E_SHAPE, "cwfa_attention_combine_f32: bad shape");
    if (B == 0 || HW == 0) return CWFA_OK;
    hipLaunchKernelGGL(attention_combine_kernel, dim3((unsigned)((HW + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, mean,
                       w1, b1, w2, b2, m, x, out, C, HW);
    CWFA_LAUNCH_CHECK("cwfa_attention_combine_f32");
    return CWFA_OK;
}
