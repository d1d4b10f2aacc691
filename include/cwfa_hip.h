/*
 * cwfa_hip.h -- C ABI of libcwfa_hip.so: hand-written HIP kernels (gfx950 / MI355X) for the
 * CWFA inverse (reconstruction) and forward-NLL hot path.
 *
 * The reference (pvjosue/CWFA) is pure Python on torch ops and has NO native boundary; each entry
 * point below therefore names the reference *Python* op sequence (file:line, relative to the
 * reference root) whose stock ATen kernels it replaces.  The Python host layer (cwfa_amd/) binds
 * these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain C: raw device pointers + sizes, no torch / C++ types.  `stream` is a hipStream_t passed
 *     as void* (NULL = the null stream).
 *   - every launch function ENQUEUES work on `stream` and returns immediately: 0 on success,
 *     <0 on error (CWFA_E_*).  Nothing aborts, nothing synchronises, nothing is allocated.
 *   - cwfa_last_error() returns a thread-local message for the last failing call.
 *   - tensors are fp32, NCHW, innermost (H,W) plane contiguous; where a `*_bs` argument exists it
 *     is the batch stride IN ELEMENTS, the channel stride is H*W (so channel-sliced views of a
 *     larger tensor are passed without a copy: Split / torch.cat never materialise).
 *   - index tables are int64 (torch.LongTensor, as the reference stores them) and are applied
 *     bit-exactly.
 */
#ifndef CWFA_HIP_H
#define CWFA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CWFA_VERSION 100

enum {
    CWFA_OK = 0,
    CWFA_E_INVAL = -1,  /* null pointer / bad enum / negative size */
    CWFA_E_SHAPE = -2,  /* shape not supported by the kernel */
    CWFA_E_ALIGN = -3,  /* pointer / stride alignment */
    CWFA_E_HIP = -4     /* HIP runtime error at launch */
};

/* soft-clamp of the multiplicative coupling coefficient: s = clamp * f(a)
 * FrEIA/modules/coupling_layers.py:50-60; all_in_one_block.py:216 (TANH) */
enum { CWFA_CLAMP_NONE = 0, CWFA_CLAMP_ATAN = 1, CWFA_CLAMP_TANH = 2, CWFA_CLAMP_SIGMOID = 3 };

/* activations usable in conv epilogues */
enum { CWFA_ACT_NONE = 0, CWFA_ACT_ELU = 1, CWFA_ACT_PRELU = 2, CWFA_ACT_GELU = 3, CWFA_ACT_RELU = 4 };

int cwfa_version(void);
const char* cwfa_last_error(void);
/* process-wide tuning options (set before packing weights; pack and launch consult the same value):
 *   "winograd_min_cout" : 3x3 convolutions with at least this many output channels use the Winograd kernels
 *                         (default 1; a value above every Cout selects the direct kernels everywhere).
 *   "winograd_2d"       : v > 0: layers with more than 64 and at least v output channels use the 2-D F(2x2,3x3) kernel
 *                         (+1..13 % on plain convolutions, slower with a load-side prologue); 0: the 1-D F(2,3) kernel
 *                         as for the narrower layers.
 *   "split_products"    : 6 (default): the split-bf16 kernels form every fp32 product from six bf16 products
 *                         (fp32-equivalent); 1: plain 16-bit operands (BASELINE.json configs[4]), one product each.
 *   "split_operand"     : 0 (default): bf16 operands; 1: fp16 operands (round to nearest even, beyond +-65504 +-inf) on the
 *                         f16 matrix-core forms, for the single-product kernels: the split 1x1 / transposed GEMM and its
 *                         input split, the split 3x3 / 7x7 and coupling-epilogue convolutions, the fused sub-network layers,
 *                         the split Conv3d, and their pack functions (a packed image is valid for the option values it was
 *                         packed under).  The valid pairs (split_products, split_operand) are (6, 0), (1, 0) and (1, 1): a call
 *                         that would make (6, 1) returns CWFA_E_INVAL, so set split_products = 1 before split_operand = 1, and
 *                         split_operand = 0 before split_products = 6.  The 3x3 weight gradient ("wgrad_split") is not affected.
 *   "wgrad_rows"        : 0: the 3x3 weight gradient always takes its first (register-staged) form.
 *   "wgrad_split"       : 1: the 3x3 weight gradient (16-byte aligned rows) runs on the bf16 matrix cores in the split
 *                         arithmetic of "split_products" (training in split / bf16 precision); 0 (default): fp32 MFMA.
 *   "split3x3_xcd_map"  : 0: (ablation) blocks of the split 3x3 kernel in plain (spatial tile, cout tile) order instead of
 *                         the XCD-aware one.
 *   "mip3_ablate"       : measurement only (results are then WRONG): mask, bit 0 / 1 / 2 drops the over-depth / over-H / over-W
 *                         reduction of cwfa_mip3_f32 (which of the three bounds the kernel); default 0.
 *   "split3x3_rows16"   : 0: (ablation) the 64-channel tiling of the split 3x3 kernel always on 8-row tiles.
 *   "reg_upsample_stages": measurement only (with a bit cleared the map is NOT computed): mask, bit 0 / 1 / 2 launches the twiddle /
 *                         row / column kernel of cwfa_reg_upsample_c64 (what each of them costs); default 7.
 * returns 0, or CWFA_E_INVAL for an unknown name or an invalid value. */
int cwfa_set_option(const char* name, int value);

/* ------------------------------------------------------------------------------------------------
 * Haar wavelets
 * ---------------------------------------------------------------------------------------------- */

/* HaarTransform1D.forward(rev=False) fused with Split.forward   INN_utils.py:151-161, graph_topology.py:73-80
 * x [B,D,H,W] -> lo [B,D/2,H,W] = (x[2i]+x[2i+1])*f,  hi = (x[2i]-x[2i+1])*f,  f = fp32(1/sqrt2).
 * lo / hi are separate views (pass out+0 and out+(D/2)*HW with the same batch stride to get the
 * reference's single [B,D,H,W] output).  Bit-exact with the reference (same two fp32 ops). */
int cwfa_haar1d_fwd_f32(const float* x, float* lo, float* hi, int B, int D, int64_t HW,
                        int64_t x_bs, int64_t lo_bs, int64_t hi_bs, void* stream);

/* HaarTransform1D.forward(rev=True) fused with Split.forward(rev=True)=torch.cat   INN_utils.py:157-161
 * x[2i] = (lo[i]+hi[i])*f, x[2i+1] = (lo[i]-hi[i])*f.  hi == NULL means hi = 0 (unused by callers today). */
int cwfa_haar1d_inv_f32(const float* lo, const float* hi, float* x, int B, int D, int64_t HW,
                        int64_t lo_bs, int64_t hi_bs, int64_t x_bs, void* stream);

/* HaarDownsampling.forward   FrEIA/modules/reshapes.py:273-300  (2x2 spatial Haar, [B,C,H,W] <-> [B,4C,H/2,W/2])
 * fac = 0.5*rebalance (fwd) or 0.5/rebalance (rev); order_by_wavelet selects channel order j*C+c vs c*4+j. */
int cwfa_haar2d_fwd_f32(const float* x, float* y, int B, int C, int H, int W, int order_by_wavelet, float fac,
                        void* stream);
int cwfa_haar2d_inv_f32(const float* y, float* x, int B, int C, int H, int W, int order_by_wavelet, float fac,
                        void* stream);

/* 3-D Haar over 2 x 2 x 2 tiles in ONE pass: the depth Haar (INN_utils.py:142-161; lo | hi halves on the channel axis)
 * followed by the spatial Haar of every band (reshapes.py:273-300), y = haar2d(haar1d(x)): x [B,D,H,W] (batch stride
 * x_bs) <-> y [B,4D,H/2,W/2] (contiguous).  order_by_wavelet / fac as cwfa_haar2d_*; bit-identical to the two-launch
 * composition; 8 bytes of traffic per element instead of 16. */
int cwfa_haar3d_fwd_f32(const float* x, float* y, int B, int D, int H, int W, int order_by_wavelet, float fac, int64_t x_bs,
                        void* stream);
int cwfa_haar3d_inv_f32(const float* y, float* x, int B, int D, int H, int W, int order_by_wavelet, float fac, int64_t x_bs,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Permutations (index gathers)
 * ---------------------------------------------------------------------------------------------- */

/* y[.., i, ..] = x[.., perm[i], ..] along axis (1 = channels, 2 = rows, 3 = columns).
 * PermuteRandom.forward fixed_transforms.py:37-41; PermuteDim.forward INN_utils.py:73-81;
 * AllInOneBlock hard permutation all_in_one_block.py:191-196 (a 0/1 1x1 conv == channel gather). */
int cwfa_gather_f32(const float* x, const int64_t* perm, float* y, int B, int C, int H, int W, int axis,
                    int64_t x_bs, int64_t y_bs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Affine coupling apply (+ fused input gather, per-channel affine, log-det, sum of squares)
 * ---------------------------------------------------------------------------------------------- */

typedef struct {
    const float* s_raw;   /* [B,C,H,W] pre-clamp multiplicative coefficient; NULL = no scaling (NICE)      */
    const float* t;       /* [B,C,H,W] additive coefficient; NULL = 0                                      */
    int64_t s_bs, t_bs;   /* batch strides (elements)                                                      */
    int clamp_kind;       /* CWFA_CLAMP_*                                                                  */
    float clamp;          /* alpha (2.0 default)                                                           */
    float pre_scale;      /* multiplies s_raw and t first (AllInOneBlock `a *= 0.1`), 1.0 otherwise        */
    int t_neg_div_sqrt2;  /* 1: t := -t / sqrt(2)  (wavelet_flow_subnetwork2D_first pass-through,
                             networks.py:671) so the torch.cat of that subnet never materialises          */
    const int64_t* perm;  /* optional gather applied to the INPUT of this stage: v_in[p] = v_prev[g(p)]    */
    int perm_axis;        /* 1 / 2 / 3 (see cwfa_gather_f32); ignored when perm == NULL                    */
    int gin;              /* 1: subtract the channel mean of s at every pixel (GIN, coupling_layers.py:355) */
} cwfa_affine_stage;

/* One coupling apply:  fwd y = exp(s)*x' + t,   rev y = (x' - t)*exp(-s),   x' = gather(x),  s = clamp*f(pre*s_raw)
 * coupling_layers.py:209-217,281-289,492-500; all_in_one_block.py:213-225.
 * x == NULL means x = 0 (z at temperature 0, CWFA.py:54-55).
 * logdet (nullable): double[B], ACCUMULATED with += sum_{c,h,w} s (fwd) or -= (rev).
 * sumsq  (nullable): double[1], ACCUMULATED with += sum y^2  (||Z||^2 of CWFA.py:970). */
int cwfa_affine_f32(const float* x, float* y, const cwfa_affine_stage* st, int rev, int B, int C, int H, int W,
                    int64_t x_bs, int64_t y_bs, double* logdet, double* sumsq, void* stream);

/* ActNorm / AllInOneBlock global affine, per channel:   invertible_resnet.py:78-81; all_in_one_block.py:181-196
 * mode 0: y = x*scale[c] + shift[c];   mode 1: y = (x - shift[c]) / scale[c];
 * optional channel gather on the input (perm, applied before the affine) or on the output
 * (perm_out: y[:, i] = v[:, perm_out[i]] of the affine result), at most one of them. */
int cwfa_channel_affine_f32(const float* x, float* y, const float* scale, const float* shift, int mode,
                            const int64_t* perm_in, const int64_t* perm_out, int B, int C, int64_t HW,
                            int64_t x_bs, int64_t y_bs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused flow chain for CAT-type steps (every s,t depends on the conditions only)
 * ---------------------------------------------------------------------------------------------- */
#define CWFA_CHAIN_MAX 8

typedef struct {
    int n_stages;
    cwfa_affine_stage stage[CWFA_CHAIN_MAX];   /* in EXECUTION order for the requested direction */
    /* Optional (both or none; device int32): the stages' channel / row gathers composed by the caller, so that a kernel
     * reads where each stage takes its s,t rows from instead of walking the permutation tables (a chain of dependent
     * loads): src_c [n_stages+1][C], src_h [n_stages+1][H]; row k < n_stages = the channel / image row at which stage k
     * reads its coefficients for OUTPUT channel / row i, row n_stages = where the travelling value starts (for
     * cwfa_chain_fwd_f32 the final permutation is part of the composition).  Used by the 16-byte row kernels of
     * cwfa_chain_inv_f32 / cwfa_chain_fwd_f32; every other entry point ignores them. */
    const int32_t* src_c;
    const int32_t* src_h;
} cwfa_chain;

/* Inverse of one whole conditional step in ONE launch:  GraphINN.forward(rev=True) over
 * [PermuteRandom^-1, (CAT^-1, Permute^-1) x n, CAT_first^-1, Split^-1(cat), HaarTransform1D^-1]
 * graph_inn.py:280-311 over the graph of networks.py:305-366.
 *   v = z (NULL = 0);  for each stage: v <- A_k^-1(gather_k(v));  x = Haar1D^-1(cat[low, v])
 * z [B,C,H,W], low [B,C,H,W] -> x [B,2C,H,W].  logdet nullable (accumulated, rev sign). */
int cwfa_chain_inv_f32(const float* z, const float* low, float* x, const cwfa_chain* ch, int B, int C, int H, int W,
                       int64_t z_bs, int64_t low_bs, int64_t x_bs, double* logdet, void* stream);

/* Per-voxel variance of x = cwfa_chain_inv_f32(z, low, ...) when the elements of z are independent with variance z_var
 * and low carries an independent per-voxel variance var_low [B,C,H,W] (NULL = 0).  `ch` as for cwfa_chain_inv_f32
 * (execution order of the inverse; src_c / src_h honoured); t is never read.
 *   a = 0;  for each stage: a <- gather_k(a) - 2*s_k;   var_v = z_var * exp(a)
 *   out[2c] = out[2c+1] = (var_low[c] + var_v[c]) * 0.5            out [B,2C,H,W]
 * std_scale == 0: out is the variance;  std_scale > 0: out = std_scale * sqrt(variance)  (the last step of a pyramid).
 * z_var and std_scale must be finite and >= 0.  z_var == 0 gives exactly var_low * 0.5. */
int cwfa_chain_inv_var_f32(const float* var_low, float* out, const cwfa_chain* ch, float z_var, float std_scale,
                           int B, int C, int H, int W, int64_t var_low_bs, int64_t out_bs, void* stream);

/* One step's term of the exact covariance of ROI means of the volume a CAT pyramid reconstructs.  `ch` is the
 * step's chain as for cwfa_chain_inv_var_f32 ([B,C,H,W] coefficients, execution order of the inverse; t, src_c, src_h never read),
 * `level` = m in 1..30 counts the steps from the finest (m = 1) so that the final volume has D = C * 2^m depths.  boxes: HOST int32
 * [R][6] = {z0,z1,y0,y1,x0,x1}, half-open, inside D x H x W (as cwfa_roi_means_f32); pairs: HOST int32 [P][2] box indices, NULL = the
 * R diagonal pairs (then P must be R).  For every pair and batch sample
 *   out[b][p] += z_var * 2^-m / (cnt1 * cnt2) * sum_c q1(c) q2(c) * sum_{(y,x) in both footprints} exp(a[b,c,y,x])
 * with a the travelling sum of cwfa_chain_inv_var_f32 and q(c) = (depths of the box in the first half of [c 2^m, (c+1) 2^m)) - (depths
 * in its second half).  out: DEVICE double [B][P], batch stride out_bs >= P, zeroed by the caller; the calls of a pyramid's steps
 * accumulate in stream order and no atomics are used, so a call is bitwise repeatable.  A pair with an empty box is set to NaN; an
 * empty footprint intersection, a channel with q1 q2 = 0 (never read) and z_var = 0 add exactly nothing.
 * dev_table (nullable): a DEVICE int32 [P][12] copy of the pairs' boxes (box of pairs[p][0], then box of pairs[p][1]): one launch for
 * any P.  NULL: the boxes travel in the kernel arguments, 64 pairs per launch.  The host tables are validated either way. */
int cwfa_chain_inv_roi_cov_f32(double* out, const cwfa_chain* ch, float z_var, int B, int C, int H, int W, int level,
                               const int32_t* boxes, int R, const int32_t* pairs, int P, const int32_t* dev_table, int64_t out_bs,
                               void* stream);

/* The counter-based generator of the samplers: Philox4x32-10 under the key (seed & 0xffffffff, seed >> 32).  Element e (the
 * contiguous linear index within ONE sample) of sample n takes word e & 3 of the block with counter
 * (g & 0xffffffff, g >> 32, sample_offset + n, stream_id), g = e >> 2; as a uniform, u = ((word >> 9) + 0.5) * 2^-23 (exact in
 * fp32, strictly inside (0, 1)).  A call over samples [0, N) therefore equals calls over [0, k) and, with sample_offset + k,
 * [k, N), whatever kernel form runs.  out [N][n] with sample stride out_ss (elements, >= n). */
int cwfa_rand_uniform_f32(float* out, int N, int64_t n, int64_t out_ss, uint64_t seed, uint32_t stream_id, uint32_t sample_offset,
                          void* stream);
/* The latent draw of sample_z_truncated (CWFA.py:47-64; utils.py:42-82 with mean 0, std 1, bounds +-temperature) in one launch:
 *   z = clamp(sqrt2f * erfinvf(E * (2u - 1)), -T, T),   E = (float)erf(T / sqrt 2) formed in double on the host
 * temperature must be > 0 (inf allowed: E = 1 and |z| stays below about 5.2). */
int cwfa_rand_trunc_normal_f32(float* out, int N, int64_t n, int64_t out_ss, float temperature, uint64_t seed, uint32_t stream_id,
                               uint32_t sample_offset, void* stream);

/* N posterior samples of one conditional step in ONE launch, the latents drawn in the kernel:
 *   x[n] = cwfa_chain_inv_f32(z[n], low[n], ch)   with z[n] drawn as by cwfa_rand_trunc_normal_f32
 * The coefficient rows of `ch` (as for cwfa_chain_inv_f32; src_c / src_h honoured) are read once for all samples; per sample one
 * low plane is read and two planes are written.  low [N][B,C,H,W] with sample stride low_ss (0: every sample shares one low, as
 * at the coarsest step), x [N][B,2C,H,W], z_out (nullable) [N][B,C,H,W]; all sample and batch strides in elements, 64-bit.
 * The latent that ARRIVES at position (b, c, h, w) of the chain's output is element e = ((b*C + c)*H + h)*W + w of the generator
 * above; z_out receives it at the position where it STARTS, so that cwfa_chain_inv_f32(z_out[n], low[n], ..) reproduces x[n]
 * (to rounding: the kernel evaluates g*z + o with the chain collapsed to one pair per element).  temperature must be > 0. */
int cwfa_chain_inv_samples_f32(const float* low, float* x, float* z_out, const cwfa_chain* ch, int N, int B, int C, int H, int W,
                               int64_t low_ss, int64_t low_bs, int64_t x_ss, int64_t x_bs, int64_t z_ss, int64_t z_bs,
                               float temperature, uint64_t seed, uint32_t stream_id, uint32_t sample_offset, void* stream);

/* Per-coefficient z-scores and NLL shares of a volume x [B,2C,H,W] under one conditional step, in ONE launch.  `ch` holds the stages
 * of the INVERSE direction, as for cwfa_chain_inv_f32 (src_c / src_h honoured).  The step gives the detail d = (x[2c] - x[2c+1]) /
 * sqrt 2 at volume position p the density of  g * z + o  with z standard normal; the pair is collapsed once per position:
 *   (a, o) = (0, 0);  for each stage: (a, o) <- gather_k(a, o);  o <- (o - t_k) * exp(-s_k);  a <- a + s_k         (g = exp(-a))
 *   z[p] = (d[p] - o[p]) * exp(a[p])        the latent that the inverse chain carries to p: the standardised residual of d[p]
 *   nll[p] = z[p]^2 / 2 - a[p]              its share of 0.5 * sum z^2 - logdet of cwfa_chain_fwd_f32 (no log 2 pi term)
 *   low[p] = (x[2c] + x[2c+1]) * fl(1 / sqrt 2)     bit-equal to cwfa_chain_fwd_f32's low
 * low, z, nll [B,C,H,W] are written at the coefficient's OWN position (nothing scatters); each is nullable and has its own batch
 * stride.  nll_sum (nullable, double [B]) ACCUMULATES the per-sample sum of nll.  At least one of the four must be given; the
 * outputs must not overlap x or one another. */
int cwfa_chain_nll_map_f32(const float* x, float* low, float* z, float* nll, const cwfa_chain* ch, int B, int C, int H, int W,
                           int64_t x_bs, int64_t low_bs, int64_t z_bs, int64_t nll_bs, double* nll_sum, void* stream);

/* The per-step maps of a pyramid as one full-resolution volume: a coefficient of level n (0 = finest) covers 2^(n+1) adjacent
 * depths at one pixel and gives each of them an equal share,
 *   out[b, d, h, w] = sum_{n < L} 2^-(n+1) * level_n[b, d >> (n+1), h, w]          level_n [B, D >> (n+1), H, W], out [B, D, H, W]
 * added finest first in fp32 (the factors are powers of two: every product is exact, so the same fp32 expression gives the same
 * bits anywhere), so that the sum of out over a sample is the sum of all levels.  1 <= L <= CWFA_NLL_MAX_LEVELS, D divisible by
 * 2^L; the levels have contiguous planes (channel stride HW) and their own batch strides. */
#define CWFA_NLL_MAX_LEVELS 8
typedef struct {
    int n;
    const float* level[CWFA_NLL_MAX_LEVELS];   /* finest first */
    int64_t bs[CWFA_NLL_MAX_LEVELS];           /* batch strides, elements */
} cwfa_nll_levels;
int cwfa_nll_compose_f32(const cwfa_nll_levels* levels, float* out, int B, int D, int64_t HW, int64_t out_bs, void* stream);

/* Forward (NLL direction) of one whole conditional step in ONE launch:
 *   (low, v) = Split(Haar1D(x));  for each stage: v <- A_k(gather_k(v));  z = gather_final(v)
 * final_perm (nullable) is the trailing PermuteRandom (networks.py:353-357).
 * logdet += sum s (per sample), sumsq += sum z^2 (CWFA.py:966-978). */
int cwfa_chain_fwd_f32(const float* x, float* low, float* z, const cwfa_chain* ch, const int64_t* final_perm,
                       int B, int C, int H, int W, int64_t x_bs, int64_t low_bs, int64_t z_bs,
                       double* logdet, double* sumsq, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 2-D convolution on fp32 MFMA (implicit GEMM, no im2col), stride 1, zero padding ks/2, groups 1
 * replaces nn.Conv2d / F.conv2d at networks.py:212-219,488-492,537,621-638; unet.py:99-104,66
 * ---------------------------------------------------------------------------------------------- */

/* number of floats of the packed weight image for a [Cout,Cin,ks,ks] filter bank */
int64_t cwfa_conv2d_packed_floats(int Cout, int Cin, int ks);
/* repack torch-layout weights [Cout,Cin,ks,ks] (device) into the kernel's tiled image (device).
 * transposed != 0: source is ConvTranspose2d layout [Cin,Cout,ks,ks] with ks==2, stride 2 (unet.py:166);
 * the packed image is then the equivalent 1x1 conv with 4*Cout outputs ordered (dy*2+dx)*Cout+co. */
int cwfa_conv2d_pack_f32(const float* w, float* packed, int Cout, int Cin, int ks, int transposed, void* stream);

typedef struct {
    const float* bias;        /* [Cout] nullable                                                          */
    int act;                  /* CWFA_ACT_* applied to (acc + bias)                                       */
    const float* prelu_alpha; /* device scalar (nn.PReLU() has ONE parameter)                             */
    const float* residual;    /* nullable, same shape as y; added AFTER act                               */
    int64_t res_bs;
    int act2;                 /* CWFA_ACT_* applied after the residual add                                */
    const float* in_scale;    /* nullable [Cin]: input is read as x*in_scale[c] + in_shift[c]             */
    const float* in_shift;    /*   (eval-mode BatchNorm of the producer folded into the load; exact with  */
                              /*    zero padding because padding is inserted after the affine)            */
    int in_affine_bs;         /* 0: in_scale/in_shift are [Cin] shared by the batch; else the per-sample
                                 stride ([B,Cin] tables: BatchNorm x dropout2d channel mask, unet.py:80,86)  */
    const float* in_add;      /* nullable, same shape as x: added after the affine (UNet skip add)        */
    int64_t in_add_bs;
    int upshuffle2;           /* 1: the Cout = 4*Co outputs are written pixel-shuffled to [B,Co,2H,2W]
                                 (ConvTranspose2d k=2 s=2 as a 1x1 conv, unet.py:166); residual/bias then
                                 index the shuffled output ([Co])                                         */
    int in_blocked8;          /* cwfa_conv3x3_split_f32 only: x is channel-blocked [B][Cin/8][H][W][8] (what
                                 cwfa_subnet_layer_split_f32 writes with layout bit 1); Cin % 8 == 0, no in_* */
    int out_blocked8;         /* y is written channel-blocked [B][Cout/8][H][W][8]: cwfa_conv2d_f32 for 1x1 banks
                                 with 33..64 outputs, bias only (the first convolution of a coupling sub-network
                                 feeding cwfa_subnet_layer_split_f32 with layout bit 0); cwfa_conv3x3_split_f32
                                 with a bias / PReLU epilogue, with in_add PReLU only (consumer: in_blocked8) */
    const float* in_cat;      /* cwfa_conv2d_f32, 1x1 banks with <= 64 outputs, no other in_*: the input is the channel
                                 concatenation cat(x, in_cat) WITHOUT materialising it (the input of a coupling
                                 sub-network, cat(half, *conditions): coupling_layers.py:74-87, all_in_one_block.py:
                                 244-247).  x holds in_cat_c1 channels; the bank is packed for Cin = in_cat_from +
                                 channels(in_cat) with zero columns in [in_cat_c1, in_cat_from), in_cat_from % 16 == 0 */
    int64_t in_cat_bs;
    int in_cat_from, in_cat_c1;
    double* out_stats;        /* cwfa_conv3x3_split_f32 only (NCHW output, bias / PReLU epilogue; with in_add PReLU only):
                                 nullable [2*Cout]; the launch ADDS (sum y, sum y^2) of its output over (B,H,W) per
                                 channel -- the train-mode BatchNorm statistics of the layer that follows the convolution (unet.py:99-107), taken
                                 from the accumulators instead of a second pass over y (cwfa_channel_stats_f32)       */
    int prelu_per_channel;    /* cwfa_conv3x3_split_f32 only: prelu_alpha points to Cout slopes, one per output channel
                                 (slope 1.0 = no activation on that channel): several filter banks that read the same
                                 input -- conv1 (+ PReLU) and downsample (plain) of the condition nets' ResidualBlocks,
                                 networks.py:212-219,229-233 -- run as ONE convolution                                 */
    double* out_sample_stats; /* cwfa_conv7x7_split_f32 with Cin <= 8 only (the few-channel form): nullable [2*B]; the launch
                                 ADDS (sum y, sum y^2) of sample b's output over (C,H,W) to entries 2b, 2b + 1 -- the
                                 statistics of the nn.LayerNorm([C,H,W]) behind the ConvNeXt block's 7x7 (networks.py:490),
                                 float64 from the first addition, taken from the values the epilogue stores instead of a
                                 second pass over y (cwfa_sample_stats_f32).  Every other entry point and form rejects it */
} cwfa_conv_opts;

int cwfa_conv2d_f32(const float* x, const float* w_packed, float* y, int B, int Cin, int H, int W, int Cout, int ks,
                    int64_t x_bs, int64_t y_bs, const cwfa_conv_opts* opts, void* stream);

/* One residual layer of the coupling sub-network (networks.py:624-631,660-665) fused into ONE launch, 64 channels:
 *     y = ELU( conv1x1( ELU( conv3x3(x) + b3 ) ) + b1 + x )
 * The 3x3 accumulators are consumed in registers as the B operand of the 1x1 MFMAs; the hidden map never exists in
 * memory.  w3_packed: cwfa_conv2d_pack_f32 image of the [64,64,3,3] filter; w1_panel: cwfa_subnet_pack1x1_f32 image
 * (4096 floats) of the [64,64,1,1] filter. */
int cwfa_subnet_pack1x1_f32(const float* w, float* panel, void* stream);
int cwfa_subnet_layer_f32(const float* x, const float* w3_packed, const float* b3, const float* w1_panel, const float* b1,
                          float* y, int B, int H, int W, int64_t x_bs, int64_t y_bs, void* stream);
/* The same layer for the training forward: additionally writes the hidden map h = ELU(conv3x3(x) + b3) [B,64,H,W] (batch
 * stride hidden_bs) that the backward needs, from the accumulators it already holds (one extra store per element). */
int cwfa_subnet_layer_tape_f32(const float* x, const float* w3_packed, const float* b3, const float* w1_panel, const float* b1,
                               float* y, float* hidden, int B, int H, int W, int64_t x_bs, int64_t y_bs, int64_t hidden_bs,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * Condition-net 3-D part:  Conv3d(1->K,3^3,pad 1) -> PReLU -> Conv3d(K->1,3^3,pad 1), fused
 * networks.py:221-225,239 on the [B,1,H,W,D] view of a [B,D,H,W] tensor (depth = channel axis).
 * w1 [K,1,3,3,3] (kh,kw,kd), b1 [K], alpha scalar, w2 [1,K,3,3,3], b2 [1].  K <= 32.
 * ---------------------------------------------------------------------------------------------- */
int cwfa_conv3d_1k1_f32(const float* x, const float* w1, const float* b1, const float* alpha, const float* w2,
                        const float* b2, float* y, int B, int D, int H, int W, int K, void* stream);
/* The same stage with fp32-equivalent arithmetic on the bf16 matrix cores (three bf16 pieces per operand, six products, fp32
 * accumulation; "split_products" = 1: plain bf16 operands): both convolutions on v_mfma_f32_16x16x32_bf16, the sum over the
 * depth taps of the second one taken through the accumulator input while a wave walks the depth axis (csrc/conv3d_split.hip).
 * Same arguments and semantics as cwfa_conv3d_1k1_f32; K <= 32. */
int cwfa_conv3d_1k1_split_f32(const float* x, const float* w1, const float* b1, const float* alpha, const float* w2,
                              const float* b2, float* y, int B, int D, int H, int W, int K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LRNN pieces (unet.py:72-113,161-195; networks.py:244-262,468-555)
 * ---------------------------------------------------------------------------------------------- */

/* per-channel batch statistics for train-mode BatchNorm2d: stats[2*C] += (sum, sumsq) over (B,H,W), double */
int cwfa_channel_stats_f32(const float* x, double* stats, int B, int C, int64_t HW, int64_t x_bs, void* stream);
/* turn (sum,sumsq,count) or running (mean,var) into scale/shift: scale = w*rsqrt(var+eps), shift = b - mean*scale
 * stats != NULL: batch statistics (biased variance);  else running_mean / running_var.
 * mask_bc (nullable, [B*C]): per-(sample,channel) multiplier (F.dropout2d keep-mask / (1-p)); scale and shift are then
 * [B*C] tables scale[b,c] = s_c*m, shift[b,c] = t_c*m; otherwise [C] (B is ignored).
 * weight / bias NULL mean 1 / 0 (so a bare mask can be turned into an input affine). */
int cwfa_bn_fold_f32(const double* stats, double count, const float* running_mean, const float* running_var,
                     const float* weight, const float* bias, float eps, const float* mask_bc, int B, float* scale,
                     float* shift, int C, void* stream);
/* train-mode buffer bookkeeping of nn.BatchNorm2d (unet.py:101-107) from the same statistics: running_mean/var updated
 * with `momentum` (unbiased variance), num_batches_tracked (int64, nullable) incremented. */
/* cwfa_bn_fold_f32 + cwfa_bn_running_update_f32 in one launch; additionally the dropout factor may be given as the raw uniform
 * draw (mask_u [B*C], drop_p, keep_scale = fp32(1 - p)): m = (u >= p) / keep_scale, F.dropout2d unet.py:80,86; zero_stats: the
 * statistics buffer is cleared for its next accumulation (cwfa_channel_stats_f32 adds into it). */
int cwfa_bn_finish_f32(double* stats, double count, float* running_mean, float* running_var, long long* num_batches_tracked,
                       float momentum, int update_running, const float* weight, const float* bias, float eps, const float* mask_bc,
                       const float* mask_u, float drop_p, float keep_scale, int B, float* scale, float* shift, int C, int zero_stats,
                       void* stream);
int cwfa_bn_running_update_f32(const double* stats, double count, float momentum, float* running_mean, float* running_var,
                               long long* num_batches_tracked, int C, void* stream);
/* F.adaptive_max_pool2d(x, (Ho,Wo)) (unet.py:79) with an optional per-channel affine applied BEFORE the max
 * (the producer's BatchNorm); also writes the affine result at full resolution to `full` (nullable; the skip). */
int cwfa_maxpool_f32(const float* x, float* y, float* full, const float* scale, const float* shift, int B, int C,
                     int H, int W, int Ho, int Wo, void* stream);
/* per-sample statistics over (C,H,W) for nn.LayerNorm([C,H,W]): stats[2*B] += (sum, sumsq), double */
int cwfa_sample_stats_f32(const float* x, double* stats, int B, int64_t CHW, void* stream);
/* y = (x - mean_b) * rstd_b * w[chw] + b[chw]   networks.py:490 (eps 1e-5) */
int cwfa_layernorm_apply_f32(const float* x, const double* stats, const float* w, const float* b, float eps,
                             float* y, int B, int64_t CHW, void* stream);
/* The tail of a ConvNeXt block (networks.py:490-503) in one pass, C <= 64, fp32 (v_mfma_f32_32x32x2_f32, k ascending):
 *   y[b,co,p] = GELU(b1[co] + sum_ci w1[co,ci] * LN(v)[b,ci,p]) + gate[b] * u[b,co,p]
 *   LN(v)[b,ci,p] = (v[b,ci,p] - mean_b) * rstd_b * lw[ci,p] + lb[ci,p], mean_b / rstd_b from stats[2b], stats[2b+1] (the float64
 *   (sum, sum of squares) over (C,H,W): cwfa_sample_stats_f32 or cwfa_conv_opts.out_sample_stats) -- cwfa_layernorm_apply_f32's bits.
 * lw, lb: the LayerNorm tables [C*HW] (required).  w1: [C][C] (torch layout, no packed image), b1 nullable.  gate: nullable [B] (drop-path factor; null = 1).  The residual u is read
 * from memory ([B,C,HW] planes, batch stride u_bs), or, with u null, formed from the block input x [B,c_in <= 8,HW]:
 *   u[b,co,p] = b0[co] + sum_ci w0[co,ci] * x[b,ci,p]   (fmaf over ci ascending from 0.0f: the fp32 1x1 kernel's bits).
 * The result equals cwfa_layernorm_apply_f32 -> cwfa_scale_channels_f32 -> cwfa_conv2d_f32 (1x1, GELU, residual) bit for bit.
 * v, u, x, y: contiguous planes with batch strides; channels beyond C (c_in) are never read or written. */
int cwfa_convnext_tail_f32(const float* v, const double* stats, const float* lw, const float* lb, float eps,
                           const float* w1, const float* b1, const float* u, const float* gate, const float* x,
                           const float* w0, const float* b0, int c_in, float* y, int B, int C, int64_t HW,
                           int64_t v_bs, int64_t u_bs, int64_t x_bs, int64_t y_bs, void* stream);
/* GlobalAttention (networks.py:249-262) fused with the LRNN combine (networks.py:552-554):
 *   att = sigmoid(W2 . relu(conv1d_k3(mean over the flattened H*W sequence) ) )
 *   out = x + m * 2 * (att - 0.5)            (m, x nullable -> out = att) */
int cwfa_attention_combine_f32(const float* mean, const float* w1, const float* b1, const float* w2, const float* b2,
                               const float* m, const float* x, float* out, int B, int C, int64_t HW, void* stream);
/* y = x*scale[b*C+c]  (F.dropout2d channel mask / drop_path; mask generated by the caller) */
int cwfa_scale_channels_f32(const float* x, const float* scale_bc, float* y, int B, int C, int64_t HW, void* stream);
/* y = a*x + b*z (elementwise; z nullable) */
int cwfa_axpby_f32(const float* x, const float* z, float a, float b, float* y, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp32-equivalent 1x1 / 3x3 convolution and ConvTranspose2d(k2,s2) on the bf16 matrix pipe (same reference ops
 * as cwfa_conv2d_f32 with ks = 1 or 3, tiles of 256 output channels: nn.Conv2d 1x1 networks.py:488-492, nn.ConvTranspose2d unet.py:166).  Each fp32 operand is
 * split exactly into three bf16 pieces, six partial products are accumulated in fp32.
 *   cwfa_split_workspace_bytes / cwfa_split_input_f32 : x [B,Cin,HW] (+ per-channel or per-(sample,channel) affine,
 *       + added tensor, as cwfa_conv_opts in_*) -> three bf16 planes in `ws` (16-byte aligned);
 *   cwfa_conv_split_packed_bytes / _pack_f32 : torch weight [Cout,Cin] (or ConvTranspose2d [Cin,Co,2,2]) -> split image;
 *   cwfa_conv_split_f32 : y = epilogue(W . x) with bias / act / residual / act2 / upshuffle2 of `opts` (in_* must be null). */
int64_t cwfa_split_workspace_bytes(int B, int Cin, int64_t HW);
int cwfa_split_input_f32(const float* x, void* ws, int B, int Cin, int64_t HW, int64_t x_bs, const float* in_scale,
                         const float* in_shift, int64_t in_affine_bs, const float* in_add, int64_t in_add_bs, void* stream);
int64_t cwfa_conv_split_packed_bytes(int Cout, int Cin, int ks);
int cwfa_conv_split_pack_f32(const float* w, void* packed, int Cout, int Cin, int ks, int transposed, void* stream);
/* 3x3 (stride 1, zero padding 1) with the same arithmetic straight from the fp32 tensor: the kernel applies the load-side
 * affine / added tensor of `opts` and splits on the way into LDS (no workspace, no extra pass); v_mfma_f32_16x16x32_bf16,
 * one wave per SIMD (csrc/conv_split3x3.hip).  packed = cwfa_conv3x3_split_pack_f32(torch weight [Cout,Cin,3,3]):
 * cwfa_conv3x3_split_packed_bytes(Cout, Cin) bytes, 16-byte aligned.  Epilogue: bias / act / residual / act2 of `opts`. */
int64_t cwfa_conv3x3_split_packed_bytes(int Cout, int Cin);
int cwfa_conv3x3_split_pack_f32(const float* w, void* packed, int Cout, int Cin, void* stream);
int cwfa_conv3x3_split_f32(const float* x, const void* w_packed, float* y, int B, int Cin, int H, int W, int Cout,
                           int64_t x_bs, int64_t y_bs, const cwfa_conv_opts* opts, void* stream);
int cwfa_conv_split_f32(const void* ws, const void* w_packed, float* y, int B, int Cin, int H, int W, int Cout, int ks, int64_t y_bs,
                           const cwfa_conv_opts* opts, void* stream);
/* 7x7 (stride 1, zero padding 3; nn.Conv2d(C, C, 7, 1, 3) of the ConvNeXt block, networks.py:488) in the same arithmetic on the same
 * kernel: 3-pixel halo, 49 taps, a 49-step period over two 16-channel chunks.  Cout <= 64; epilogue: bias only; no in_* prologue.
 * Few input channels (the ConvNeXt 1x1 + 7x7 composed into one 7x7 over the block's inputs and a ones channel) take shorter forms;
 * the three entry points agree on them by Cin alone:
 *   Cin <= 8:        a kernel of its own whose K = 32 step is four (8-channel, tap) units: 13 steps, image of 13 slices
 *                    [step][piece 3][k group 4][64][8] (group g of step s = tap 4 s + g); the input tile is staged once per block;
 *   9 <= Cin <= 16:  the kernel and image of Cin >= 17 (49 slices), of which only the 25 steps that touch the one chunk are run.
 * A bank packed for Cin' inputs may be launched with any Cin that selects the same form (channels >= Cin read as 0.0). */
int64_t cwfa_conv7x7_split_packed_bytes(int Cout, int Cin);
int cwfa_conv7x7_split_pack_f32(const float* w, void* packed, int Cout, int Cin, void* stream);
int cwfa_conv7x7_split_f32(const float* x, const void* w_packed, float* y, int B, int Cin, int H, int W, int Cout,
                           int64_t x_bs, int64_t y_bs, const cwfa_conv_opts* opts, void* stream);

/* The LAST convolution of a coupling sub-network (3x3, 64 -> 2n channels: [s_raw | t], networks.py:633-638) with the affine
 * coupling applied from its accumulators -- s and t never reach memory:
 *     fwd:  y = x * exp(s) + t            rev:  y = (x - t) * exp(-s)            logdet[b] += (rev ? -1 : +1) * sum s
 *     s = soft_clamp(pre_scale * s_raw), t <- pre_scale * t      (coupling_layers.py:50-60,87-110; all_in_one_block.py:206-224)
 * x / y: the ACTIVE half [B,n,H,W] of the block (planes contiguous, batch strides x_bs / y_bs; may be the same tensor).
 * The filter bank is packed with its rows interleaved so that s_j and t_j of a pixel land in the same lane:
 *     cwfa_couple_rows(n, rows): rows[r] = source row (0..2n-1) of packed row r, or -1 (zero row), r < cwfa_couple_rows(n, NULL)
 *     w' = w[rows] (zeros for -1), bias' likewise;  packed = cwfa_conv3x3_split_pack_f32(w', Cout = that row count)
 * n <= 64.  logdet nullable (float64[B], accumulated). */
typedef struct {
    const float* x;
    float* y;
    int64_t x_bs, y_bs;
    int n;                      /* channels of the active half = half the outputs of the bank                           */
    int clamp_kind;             /* CWFA_CLAMP_*                                                                          */
    float clamp, pre_scale;
    int rev;
    double* logdet;
    int in_blocked8;            /* the convolution's input is channel-blocked (see cwfa_conv_opts.in_blocked8)           */
} cwfa_couple;
int cwfa_couple_rows(int n, int* rows);
int cwfa_conv3x3_split_couple_f32(const float* x, const void* w_packed, const float* bias_rows, int B, int Cin, int H, int W,
                                  int64_t x_bs, const cwfa_couple* cp, void* stream);

/* The fused sub-network layer  y = ELU(W1 . ELU(conv3x3(x, W3) + b3) + b1 + x), 64 channels (networks.py:624-631,660-665)
 * with BOTH convolutions on the split-bf16 core (three bf16 pieces per fp32 operand, six products, fp32 accumulation;
 * `split_products` = 1: plain bf16 operands), one persistent launch (csrc/conv_split_layer.hip).
 *   packed = cwfa_subnet_layer_split_pack_f32(w3 [64,64,3,3], w1 [64,64,1,1]): cwfa_subnet_layer_split_packed_bytes() bytes,
 *   16-byte aligned, 40 slices (36 of the 3x3 bank by (chunk of 16 input channels, tap), 4 of the 1x1 bank). */
int64_t cwfa_subnet_layer_split_packed_bytes(void);
int cwfa_subnet_layer_split_pack_f32(const float* w3, const float* w1, void* packed, void* stream);
int cwfa_subnet_layer_split_f32(const float* x, const void* packed, const float* b3, const float* b1, float* y, int B, int H,
                                int W, int64_t x_bs, int64_t y_bs, int layout, void* stream);
/* The FIRST layer of a sub-network in its composed form.  The 1x1 convolution in front of the three layers (networks.py:621-623,
 * 641-643) and the layer's 3x3 are both linear with nothing in between, so conv3x3(conv1x1(u) + b0) = conv3x3'(u | 1) with
 * W' = W3 o [W0 | b0] over u's channels and a constant-one channel (exact under zero padding: padded ones carry no bias): K = 9 x 32
 * instead of 9 x 64 -- half the convolution steps of the layer.  u: [B, u_ch <= 32, H, W] NCHW INCLUDING the ones channel;
 * x = conv1x1(u) + b0 (the residual, layout bit 0); packed = cwfa_subnet_layer_first_pack_f32(w3c [64,32,3,3] the composed bank,
 * zero in unused input channels; w1 [64,64,1,1]; w0c nullable): cwfa_subnet_layer_first_packed_bytes() bytes.
 * With w0c = [W0 | b0 | 0] ([64,32], the 1x1 bank over u's channels and the ones channel) in the packed image and x == NULL the
 * residual is not read either: the layer's 1x1 phase takes it as a third k step, [W1 | W0c] . [h ; u], from u's values at the tile's
 * pixels -- the sub-network's first 1x1 launch and its 64-channel map never exist.  SHORT form (pack with short_form = 1, launch
 * with layout bit 2 = 4, x == NULL, u_ch <= 16 = one 16-channel chunk): five instead of nine convolution steps per tile -- the steps
 * that pair only taps of the all-zero second chunk are not run. */
int64_t cwfa_subnet_layer_first_packed_bytes(void);
int cwfa_subnet_layer_first_pack_f32(const float* w3c, const float* w1, const float* w0c, int short_form, void* packed, void* stream);
int cwfa_subnet_layer_first_f32(const float* u, const float* x, const void* packed, const float* b3, const float* b1, float* y, int B,
                                int u_ch, int H, int W, int64_t u_bs, int64_t x_bs, int64_t y_bs, int layout, void* stream);
/* Tape form (training forward, SURVEY.md 8f row 1 / CWFA.py:966-1006): the same launch also writes the hidden map
 * h = ELU(conv3x3(x) + b3) [B,64,H,W] the backward needs, from the registers that hold it as the 1x1's operand.  NCHW maps. */
int cwfa_subnet_layer_split_tape_f32(const float* x, const void* packed, const float* b3, const float* b1, float* y, float* hid, int B,
                                     int H, int W, int64_t x_bs, int64_t y_bs, int64_t hid_bs, void* stream);
/* The OUTPUT convolution of a coupling sub-network, y = conv3x3(x, w) + bias with 64 -> Cout <= 48 channels (networks.py:632, 666),
 * as the conv phase of the layer above: the same persistent tile walk, LDS image and weight ring, ceil(Cout / 16) m-tiles wide,
 * with a plain NCHW store (csrc/conv_split_out.hip).  packed = cwfa_conv3x3_out_split_pack_f32(w [Cout,64,3,3]):
 * cwfa_conv3x3_out_split_packed_bytes(Cout) bytes (-1: Cout not in 1..48), 16-byte aligned, in the operand format active at pack
 * time.  bias [Cout] may be NULL.  y: Cout planes per sample, batch stride y_bs (a channel slice of a larger tensor is fine: nothing
 * outside those planes is written); in_blocked: x is a channel-blocked map (see `layout` below). */
int64_t cwfa_conv3x3_out_split_packed_bytes(int Cout);
int cwfa_conv3x3_out_split_pack_f32(const float* w, void* packed, int Cout, void* stream);
int cwfa_conv3x3_out_split_f32(const float* x, const void* packed, const float* bias, float* y, int B, int H, int W, int Cout,
                               int64_t x_bs, int64_t y_bs, int in_blocked, void* stream);
/* layout: bit 0 = x, bit 1 = y is CHANNEL-BLOCKED, [B][8 blocks][H][W][8 channels] (same size and batch strides as NCHW, 16-byte
 * aligned), instead of NCHW planes.  The maps between the layers of one sub-network are private to it; blocked, a staging entry
 * of the kernel (8 channels of a pixel) is two 16-byte loads instead of eight 4-byte ones and the four channels a lane holds for
 * a pixel leave as one 16-byte store (the 4-byte stores of the NCHW form held 15 % of a launch).  The consumer of a blocked map:
 * this function with bit 0, or cwfa_conv3x3_split_f32 / cwfa_conv3x3_split_couple_f32 with `in_blocked8`. */

/* ------------------------------------------------------------------------------------------------
 * Lenslet views (the step before the path): XLFMDatasetFull.extract_views XLFMDataset.py:212-242 followed by the
 * normalisation of CWFA.py:796-797.  image [B,1,Hs,Ws] (batch stride image_bs), coords_yx int32 [nviews][2] (device),
 * views [B,nviews,sh,sw]: window of sh x sw around each lenslet, clipped to the image, the clipped patch in the
 * bottom-right corner of a zero view, then (v - mean) / stdv (mean 0, stdv 1 = the plain extraction). */
int cwfa_extract_views_f32(const float* image, const int* coords_yx, float* views, int B, int Hs, int Ws, int nviews, int sh,
                           int sw, float mean, float stdv, int64_t image_bs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the flow-step training loss (what torch autograd does under
 * `scaler.scale(full_loss).backward()` CWFA.py:1002-1006 for the NLL term of CWFA.py:966-978)
 * ---------------------------------------------------------------------------------------------- */

/* Gradient buffers of a chain: for stage k (same order as the cwfa_chain handed to cwfa_chain_fwd_f32) ds[k] receives
 * dL/d s_raw and dt[k] dL/d t (the tensors the sub-network produced), NULL = not wanted. */
typedef struct {
    float* ds[CWFA_CHAIN_MAX];
    float* dt[CWFA_CHAIN_MAX];
    int64_t ds_bs[CWFA_CHAIN_MAX], dt_bs[CWFA_CHAIN_MAX];
} cwfa_chain_grads;

/* L = gscale * 0.5 * sum z^2 - ldscale * sum_b logdet_b (+ <gz, z> for an upstream gradient gz, nullable), z the output
 * of cwfa_chain_fwd_f32 with the same chain / final_perm.  No stored activations: every stage input is recomputed by
 * inverting the stage.  gv0 (nullable) receives dL/d(detail band entering the chain).  accumulate != 0: the stage
 * gradients are ADDED to the buffers.  gld (nullable, float[B]): an upstream gradient dL/d(logdet_b) per sample, added to the
 * uniform -ldscale (what torch autograd hands the backward of `log_jac_det.mean()`, CWFA.py:978). */
int cwfa_chain_bwd_f32(const float* z, const float* gz, const cwfa_chain* ch, const cwfa_chain_grads* grads,
                       const int64_t* final_perm, float* gv0, int B, int C, int H, int W, int64_t z_bs, int64_t gz_bs,
                       int64_t gv0_bs, float gscale, float ldscale, int accumulate, const float* gld, void* stream);

/* Backward of the reconstruction term (CWFA.py:952-959: F.l1_loss / F.mse_loss(curr_gt, upsampled_vol)) through the
 * INVERSE pass xhat = cwfa_chain_inv_f32(z, low, ...) (CWFA.py:911): L = gscale' * sum |xhat - gt|^p, p = loss_kind
 * (1: gscale = weight/numel, 2: gscale = 2*weight/numel).  `ch` is the FORWARD-order chain (as for cwfa_chain_fwd_f32);
 * the gradients go to the same buffers as cwfa_chain_bwd_f32's (accumulate != 0: added) since both passes use the same
 * coefficients.  loss_sum (nullable, double[1]) += sum |xhat - gt|^p.  No stored activations.
 * loss_kind = 0: `gt` holds an upstream gradient dL/dxhat itself (torch autograd; scaled by gscale).  gz_out / glow_out
 * (nullable, contiguous [B,C,H,W]): dL/d(latent input z) and, for loss_kind 0, dL/d(low) of the inverse pass. */
int cwfa_chain_inv_bwd_f32(const float* xhat, const float* gt, const cwfa_chain* ch, const cwfa_chain_grads* grads, int B, int C,
                           int H, int W, int64_t xhat_bs, int64_t gt_bs, float gscale, int loss_kind, int accumulate,
                           double* loss_sum, float* gz_out, float* glow_out, void* stream);

/* Backward of ONE affine stage y = cwfa_affine_f32(x, st, rev) without a gather (torch autograd of the coupling blocks that are
 * not part of a fused chain: coupling_layers.py:124-437, all_in_one_block.py:206-224): g = dL/dy, gld (nullable, float[B]) =
 * dL/d(logdet_b); writes dL/dx, dL/d s_raw, dL/d t (each nullable, contiguous [B,C,H,W]).  GIN stages included. */
int cwfa_affine_bwd_f32(const float* x, const float* g, const cwfa_affine_stage* st, int rev, int B, int C, int H, int W,
                        int64_t x_bs, int64_t g_bs, const float* gld, float* gx, float* gs_raw, float* gt_raw, void* stream);

/* Weight gradient of a stride-1, zero-padded ("same") convolution, ks = 1 or 3, on the fp32 matrix cores:
 *   dw[co][ci][ky][kx] = beta * dw + sum_{b,y,x} dy[b][co][y][x] * x[b][ci][y+ky-ks/2][x+kx-ks/2]     (torch layout)
 * and, with db != NULL, the bias gradient db[co] = beta * db + sum_{b,y,x} dy[b][co][y][x] from the same pass over dy.
 * x [B,Cin,H,W] (batch stride x_bs), dy [B,Cout,H,W] (dy_bs).  workspace: cwfa_conv2d_wgrad_workspace_bytes() bytes
 * (per-worker partial filter banks, summed in a fixed order: the result is deterministic). */
int64_t cwfa_conv2d_wgrad_workspace_bytes(int B, int Cin, int H, int W, int Cout, int ks);
int cwfa_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, float* db, void* workspace, int B, int Cin, int H, int W,
                          int Cout, int ks, int64_t x_bs, int64_t dy_bs, float beta, void* stream);

/* ELU backward from the layer output a = ELU(q):  y = g * (a > 0 ? 1 : a + 1) (+ add, nullable).  n elements per sample
 * (multiple of 4), batch strides in elements. */
int cwfa_elu_bwd_f32(const float* g, const float* a, const float* add, float* y, int B, int64_t n, int64_t g_bs, int64_t a_bs,
                     int64_t add_bs, int64_t y_bs, void* stream);

/* Backward of the condition net's 3-D stage y = W2 * PReLU(W1 * x + b1) + b2 (Conv3d 1 -> K -> 1 over (H, W, depth),
 * networks.py:221-225,239; x, y, dy: [B,D,H,W] with the depth axis as channel axis; w1 [K,1,3,3,3], w2 [1,K,3,3,3]) in
 * separate passes over a materialised hidden volume q / m [B,K,D,H,W]:
 *   hidden_fwd: q = W1 * x + b1;   hidden_bwd: m = (W2^T * dy) . PReLU'(q), dalpha (nullable, double[1]) += sum (W2^T*dy).min(q,0);
 *   input_bwd:  dx = sum_k W1[k]^T * m[k];
 *   wgrad: out32[k][tap] = beta*out32 + sum_p act(a[k][p]) * src[p + sign*(tap-1)] (tap < 27; column 27 = sum_p act(a[k][p])
 *          when want_bias), act = PReLU(alpha) if alpha != NULL -- dW2 = wgrad(a = q, alpha, src = dy, sign = -1),
 *          dW1 | db1 = wgrad(a = m, src = x, sign = +1, want_bias).  K <= 32; out32 is a [32][32] float buffer. */
int cwfa_conv3d_hidden_fwd_f32(const float* x, const float* w1, const float* b1, float* q, int B, int D, int H, int W, int K,
                               void* stream);
int cwfa_conv3d_hidden_bwd_f32(const float* dy, const float* w2, const float* q, const float* alpha, float* m, double* dalpha,
                               int B, int D, int H, int W, int K, void* stream);
int cwfa_conv3d_input_bwd_f32(const float* m, const float* w1, float* dx, int B, int D, int H, int W, int K, void* stream);
int64_t cwfa_conv3d_wgrad_workspace_bytes(int B, int D, int H, int W);
int cwfa_conv3d_wgrad_f32(const float* a, const float* src, const float* alpha, float* out32, void* workspace, int B, int D, int H,
                          int W, int K, int sign, int want_bias, float beta, void* stream);

/* PReLU backward (single alpha > 0) from the layer output o = PReLU(q):  y = g * (o > 0 ? 1 : alpha),
 * dalpha (nullable, double[1]) += sum g * min(q, 0).  n elements per sample, batch strides in elements. */
int cwfa_prelu_bwd_f32(const float* g, const float* o, const float* alpha, float* y, double* dalpha, int B, int64_t n, int64_t g_bs,
                       int64_t o_bs, int64_t y_bs, void* stream);

/* Backward pieces of the UNet (unet.py:72-113,161-195) with train-mode BatchNorm (CWFA.py:532):
 *   plane_affine: y = x * scale[(b,)c] + shift[(b,)c] (+ add)  (per_sample != 0: [B,C] tables) -- the BatchNorm (x dropout mask)
 *                 output as a tensor (the inference path applies it on load inside the next convolution);
 *   bn_bwd_stats: stats[2c] += sum g*m, stats[2c+1] += sum g*m*y over (B,H,W), m = mask_bc[b][c] or 1 (double[2C], zeroed by caller);
 *   bn_act_bwd:   out = (A[(b,)c]*g + Bc[c] + Cc[c]*y) * PReLU'(y) with y = PReLU(q) the conv output (alpha NULL: no activation),
 *                 dalpha (nullable) += sum (...)*min(q,0) -- A, Bc, Cc folded by the caller from the statistics;
 *   maxpool2_bwd: g_full = (first maximum of each 2x2 window of `full` ? g_pool : 0) + g_skip (nullable). */
int cwfa_plane_affine_f32(const float* x, const float* scale, const float* shift, int per_sample, const float* add, float* y, int B,
                          int C, int64_t HW, int64_t x_bs, int64_t add_bs, int64_t y_bs, void* stream);
int cwfa_bn_bwd_stats_f32(const float* g, const float* y, const float* mask_bc, double* stats, int B, int C, int64_t HW, int64_t g_bs,
                          int64_t y_bs, void* stream);
int cwfa_bn_act_bwd_f32(const float* g, const float* y, const float* A, int per_sample, const float* Bc, const float* Cc,
                        const float* alpha, float* out, double* dalpha, int B, int C, int64_t HW, int64_t g_bs, int64_t y_bs,
                        int64_t out_bs, void* stream);
int cwfa_maxpool2_bwd_f32(const float* full, const float* g_pool, const float* g_skip, float* g_full, int B, int C, int H, int W,
                          void* stream);

/* Backward pieces of the LRNN's mean-volume branch (ConvNeXt networks.py:468-503, GlobalAttention :244-262, combine :552-554):
 *   gelu:          mode 0: y = GELU(p) + other (nullable);  mode 1: y = other * GELU'(p)                       (n elements)
 *   layernorm_bwd: LayerNorm over the n = C*H*W elements of each sample, y = xhat*w + b with xhat = (v - mean[b])*invstd[b]:
 *                  gv = dL/dv, dw += sum_b g*xhat, db += sum_b g (dw, db ACCUMULATED); stats: double[2B] scratch, zeroed by the caller;
 *   attention_bwd: out = x + 2 m (att - 0.5), att = sigmoid(W2 relu(W1 *3 mean + b1) + b2) over the flattened H*W sequence
 *                  (C <= 8): gm = dL/dm, pgrad (double[C*C*3 + C + C*C + C], accumulated) = dL/d[w1 | b1 | w2 | b2]; dL/dx = g. */
int cwfa_gelu_f32(const float* p, const float* other, float* y, int64_t n, int mode, void* stream);
int cwfa_layernorm_bwd_f32(const float* g, const float* v, const float* w, const float* mean, const float* invstd, double* stats,
                           float* gv, float* dw, float* db, int B, int64_t n, void* stream);
int cwfa_attention_bwd_f32(const float* mean, const float* w1, const float* b1, const float* w2, const float* b2, const float* m,
                           const float* g, float* gm, double* pgrad, int B, int C, int64_t HW, void* stream);

/* The evaluation pass behind every reconstructed volume (CWFA.py:1032-1117): compute_INN_step_performance (CWFA.py:98-132) with
 * psnr (utils.py:380-394), volume_2_projections (utils.py:281-327) and the reductions of corr_coeff_3D (CWFA.py:240-379).
 * Streaming kernels over fp32 [B, D, H, W] tensors, n = D*H*W elements per sample, contiguous per sample, `*_bs` the batch
 * stride in elements.  Inputs are assumed finite (no NaN propagation).  They clear their own outputs and workspaces on `stream`.
 *
 * cwfa_eval_affine (host struct, NULL = none): every element is read as (v * scale) * std - mean, scale = 2^-step -- the
 * reference's `x / 2**step`, `x*std - mean` (CWFA.py:112-117) bit for bit, so the raw volumes need not be materialised.
 *
 *   volume_extrema: out[B][CWFA_EXTREMA_STRIDE] = {min a, max a, min|a|, max|a|, the same four of b, min|a-b|, max|a-b|, 0, 0}
 *                   (b nullable: slots 4..9 are 0).  Exact.  workspace: B * cwfa_eval_splits(B, n) * 10 floats.
 *   volume_metrics: out[B][4] (double) = {sum (g-p)^2, sum g, sum |g - p~|, #{p < thr}} with p~ = (p < thr ? 0 : p), p and g
 *                   read through the affine and then less pred_offset / gt_offset (`normaliaze_before_metrics`).  thr = -inf:
 *                   no mask.  workspace: B * cwfa_eval_splits(B, n) * 4 doubles; the sums are added in a fixed order
 *                   (bitwise reproducible).
 *   mip3:           the maximum projections of v = |a| (b NULL) or |a-b|: zproj [B,H,W] over depth, xproj [B,W,D] over H,
 *                   yproj [B,H,D] over W, gmin[B] = min v -- one read.  triple != 0: the three sets for |a|, |b|, |a-b| in the
 *                   same read, each output [3][B]...  cwfa_eval_post (one-image form only, NULL = none): the maps of
 *                   utils.py:295-303 applied to v before projecting: normalize: v = (v - norm_sub) / norm_div; threshold:
 *                   (v - vol_min) < lower -> 0, then (v - vol_min) > upper -> clamp_value.  Exact, bitwise reproducible.
 *   projection_compose: utils.py:305-325 for scaling_factors [1, 1, depth_scale]: out [B, H + D*depth_scale + border,
 *                   W + D*depth_scale + border] filled with *fill (device scalar: z_projection.min()), nearest replication
 *                   along depth, optional scale-bar lines.  H == W (the reference's size=[.., vol_size[-3]] fits no other).
 *   roi_means:      out[N][T] (double) = mean of x[t, z0:z1, y0:y1, x0:x1] for the N boxes {z0,z1,y0,y1,x0,x1} (HOST int32
 *                   [N][6], inside the volume; an empty box gives NaN).  x: [T, D, H, W] with time stride t_stride.
 *   select_positive: *value = the k-th smallest (k = 0 ..) of the strictly positive elements, k = -1: their lower median
 *                   (k = (count - 1) / 2, torch's convention); *count = the number of positive elements; k >= count gives NaN.
 *                   Radix selection on the bit patterns, 64-bit counters: exact.  workspace: CWFA_SELECT_WORKSPACE_BYTES device bytes.
 *   select_nonzero: the same over the elements != 0 of either sign (+0.0 and -0.0 are both excluded), ordered by value:
 *                   `Tmp[Tmp != 0].median()` of utils.py:702-703.  Inputs are assumed free of NaN. */
#define CWFA_EXTREMA_STRIDE 12
#define CWFA_EVAL_MAX_SPLITS 2048
#define CWFA_SELECT_WORKSPACE_BYTES 8448
typedef struct {
    int enabled;
    float scale, std, mean;
} cwfa_eval_affine;
typedef struct {
    int normalize, threshold;
    float norm_sub, norm_div, vol_min, lower, upper, clamp_value;
} cwfa_eval_post;
/* blocks per sample of the extrema / metrics kernels for B samples of n elements (<= CWFA_EVAL_MAX_SPLITS, about 2048 / B): sizes
 * their workspaces; 0 for an empty problem, CWFA_E_INVAL for a negative size */
int64_t cwfa_eval_splits(int B, int64_t n);
int cwfa_volume_extrema_f32(const float* a, const float* b, float* out, float* workspace, int B, int64_t n, int64_t a_bs,
                            int64_t b_bs, const cwfa_eval_affine* affine, void* stream);
int cwfa_volume_metrics_f32(const float* pred, const float* gt, double* out, double* workspace, int B, int64_t n, int64_t pred_bs,
                            int64_t gt_bs, const cwfa_eval_affine* affine, float pred_offset, float gt_offset, float thr,
                            void* stream);
int cwfa_mip3_f32(const float* a, const float* b, float* zproj, float* xproj, float* yproj, float* gmin, int B, int D, int H, int W,
                  int64_t a_bs, int64_t b_bs, int triple, const cwfa_eval_affine* affine, const cwfa_eval_post* post, void* stream);
int cwfa_projection_compose_f32(const float* zproj, const float* xproj, const float* yproj, const float* fill, float* out, int B,
                                int D, int H, int W, int depth_scale, int border, int scale_bars, void* stream);
int cwfa_roi_means_f32(const float* x, const int32_t* boxes, double* out, int T, int D, int H, int W, int N, int64_t t_stride,
                       void* stream);
int cwfa_select_positive_f32(const float* x, int B, int64_t n, int64_t x_bs, int64_t k, float* value, int64_t* count,
                             void* workspace, void* stream);
int cwfa_select_nonzero_f32(const float* x, int B, int64_t n, int64_t x_bs, int64_t k, float* value, int64_t* count,
                            void* workspace, void* stream);

/* The data preparation pass in front of every run: load_XLFM_data (utils.py:187-220) with load_process_volume (:128-184),
 * crop_volume_center (:105-126) and fast_quantile (:84-102), the frame clean-up of XLFMDatasetFull (XLFMDataset.py:101-104,
 * 160-162) and the statistics of ConcatDataset (XLFMDataset.py:293-395).  Streaming kernels; every fp32 operation is rounded
 * separately, in the reference's order.  Inputs are assumed free of NaN except where stated.
 *
 *   prep_volumes:  x fp16 [N,D,H0,W0] -> out [N,D,H,W] (fp32, or fp16 with out_f16), the crop x[:, :, off_h:off_h+H, off_w:off_w+W]
 *                  with the threshold step of load_process_volume on the fp16 values (compare in fp32, store fp16, widen):
 *                  VOL_NONE; VOL_TWO: v < t0 -> 0, then v >= t1 -> t1 (t1 an fp16 value); VOL_LE: v <= t0 -> 0; VOL_MAXNORM:
 *                  q = fp16(v / max) (fp32 quotient, round to nearest even), q < t0 -> 0, max taken over the cropped region by a
 *                  pass of its own; VOL_MAX_ONLY: that pass alone (out may be NULL).  maxbuf: 2 device floats (needed by the last
 *                  two modes), maxbuf[1] receives the maximum.
 *   prep_frames:   x fp32 [N,h,w] -> out fp32 [N,S0,S1]: out[n,r,c] = clean(x[n, r+off_y, c+off_x]), 0 outside the source;
 *                  clean: NaN -> 0, clip to [0, 50000], round trip through fp16 (round to nearest even).
 *   histogram:     counts[bins] (int64) of x by torch.histogram's CPU bin rule for the range [lo, hi] and the device table of
 *                  bins + 1 fp32 edges (torch.linspace(lo, hi, bins + 1)); elements outside [lo, hi] are not counted.
 *                  accumulate != 0 adds to the existing counts (chunked input).  Exact.  bins <= CWFA_PREP_MAX_BINS, lo < hi.
 *   prep_apply:    in place: PREP_CLAMP_ZERO: x > a -> a (flags bit 0), then x < b -> 0 (flags bit 1); PREP_SUB_DIV: (x - a) / b;
 *                  PREP_DIV_MUL: x / a * b.
 *   moments:       out[3] (double) = {sum (x - c), sum (x - c)^2, n}; accumulate != 0 adds to the existing three.  Float64 sums
 *                  added in a fixed order (bitwise reproducible).  workspace: CWFA_PREP_MOMENTS_WORKSPACE device doubles.
 *   stack_mean_std: mean[m], std[m] (fp32) over the N samples of x [N, m] (sample stride x_ss elements): float64 sums centred
 *                  on the first sample, unbiased std (N = 1: NaN). */
#define CWFA_PREP_MAX_BINS 10239 /* counts + edges of one block: 81916 bytes of LDS, two blocks per CU */
#define CWFA_PREP_MOMENTS_WORKSPACE 4096
enum { CWFA_PREP_VOL_NONE = 0, CWFA_PREP_VOL_TWO = 1, CWFA_PREP_VOL_LE = 2, CWFA_PREP_VOL_MAXNORM = 3, CWFA_PREP_VOL_MAX_ONLY = 4 };
enum { CWFA_PREP_CLAMP_ZERO = 0, CWFA_PREP_SUB_DIV = 1, CWFA_PREP_DIV_MUL = 2 };
int cwfa_prep_volumes_f16(const void* x, void* out, float* maxbuf, int N, int D, int H0, int W0, int H, int W, int off_h, int off_w,
                          int mode, float t0, float t1, int out_f16, void* stream);
int cwfa_prep_frames_f32(const float* x, float* out, int N, int h, int w, int S0, int S1, int off_y, int off_x, void* stream);
int cwfa_histogram_f32(const float* x, int64_t n, float lo, float hi, const float* edges, int bins, int64_t* counts, int accumulate,
                       void* stream);
int cwfa_prep_apply_f32(float* x, int64_t n, int mode, float a, float b, int flags, void* stream);
int cwfa_moments_f64(const float* x, int64_t n, double c, double* out, double* workspace, int accumulate, void* stream);
int cwfa_stack_mean_std_f32(const float* x, float* mean, float* std, int N, int64_t m, int64_t x_ss, void* stream);

/* The parameter update: `scaler.step(optimizer)` / `optimizer.step()` of CWFA.py:1011-1027 with the reference's optimiser, Lion
 * (CWFA.py:24,381,608-610; Chen et al. 2023, decoupled weight decay), INCLUDING what torch's GradScaler does around it: the
 * unscale pass over every gradient and the skip of the step when a gradient holds inf / NaN (CWFA.py:613,1011-1027).
 * One launch updates every tensor of the table.  Per element, with g' = g / *grad_scale (g' = g for grad_scale == NULL):
 *     p <- p * (1 - lr * wd);   u = sign(beta1 * m + (1 - beta1) * g')  (sign(0) = 0);   p <- p - lr * u;
 *     m <- beta2 * m + (1 - beta2) * g'
 * every fp32 operation rounded separately, 1 - beta and 1 - lr * wd formed in fp32 on the host.
 *   tab:        HOST struct: n <= CWFA_LION_MAX_TENSORS entries (p, g, m, numel) of fp32 device tensors, contiguous, 4-byte aligned,
 *               numel < 2^31; entries with numel == 0 are skipped (their pointers may be NULL).  The table is copied into the
 *               kernel's arguments: nothing is allocated or uploaded, the caller issues one call per chunk of tensors.
 *   grad_scale: nullable DEVICE scalar, read by the kernel.
 *   found_inf:  nullable DEVICE scalar, read by the kernel: if *found_inf != 0 the launch writes nothing.
 * The launch writes p and m only.  Tensors whose p, g and m are all 16-byte aligned move on 16-byte loads and stores, the others
 * and every ragged end element by element.  A block works on CWFA_LION_BLOCK_ELEMS consecutive elements of one tensor.
 * n == 0 or no elements at all: returns 0 without a launch. */
#define CWFA_LION_MAX_TENSORS 96
#define CWFA_LION_BLOCK_ELEMS 4096
typedef struct {
    float* p;        /* parameter, updated in place              */
    const float* g;  /* gradient (scaled by *grad_scale), read   */
    float* m;        /* momentum (`exp_avg`), updated in place   */
    int64_t numel;
} cwfa_lion_tensor;
typedef struct {
    int n;
    cwfa_lion_tensor t[CWFA_LION_MAX_TENSORS];
} cwfa_lion_table;
int cwfa_lion_step_f32(const cwfa_lion_table* tab, float lr, float beta1, float beta2, float weight_decay, const float* grad_scale,
                       const float* found_inf, void* stream);

/* The weighted-MSE training loss `wL2` (losses.py:477-500; CWFA.py:936-959): the squared error over the elements that are brighter
 * than ths_perc of the range in BOTH tensors,
 *     m_o = (o - min o) > (max o - min o) * ths_perc,   m_t likewise for t      (every operation rounded to fp32, as the reference)
 *     out[0] = sum (o - t)^2 m_o m_t   (float64: exact differences, partial sums added in a fixed order -- bitwise reproducible)
 *     out[1] = #{m_o and m_t}          (exact)
 *     grad[i] = (2 gscale) (o_i - t_i) inside both masks, +0.0f outside: d(gscale * out[0]) / d output; the target's is its negative.
 * One streaming pass over n contiguous elements (any n): output and target read once, grad written once; 16-byte accesses where
 * output, target and grad are 16-byte aligned, element by element otherwise and at the ragged end.
 *   extrema:   DEVICE row of cwfa_volume_extrema_f32(a = output, b = target, B = 1 over all n elements): slots 0, 1, 4, 5 = min o,
 *              max o, min t, max t are read by the kernel -- nothing goes through the host (a caller on several ranks reduces those
 *              four between the two launches).
 *   grad:      nullable: no map is written.
 *   out:       2 device doubles, written (not accumulated).
 *   workspace: cwfa_wmse_workspace_bytes(n) device bytes, 8-byte aligned; no clearing needed.
 * Nothing is allocated, nothing synchronises.  n == 0: out is zeroed, no launch.  Inputs are assumed finite. */
int64_t cwfa_wmse_workspace_bytes(int64_t n);
int cwfa_wmse_loss_f32(const float* output, const float* target, const float* extrema, float ths_perc, float gscale, float* grad,
                       double* out, void* workspace, int64_t n, void* stream);

/* Richardson-Lucy deconvolution: everything between the FFTs of XLFMDeconv (utils.py:630-738), fft_conv (:480-510) and
 * fft_conv_split (:513-550) with batch_fftshift2d_real / roll_n (:451-477).  The FFTs stay with the caller (rocFFT).  Streaming
 * kernels, 64-bit offsets, 16-byte accesses where every pointer is 16-byte aligned and the shapes allow, element by element
 * otherwise.  Every fp32 operation is rounded separately.  Nothing is allocated, nothing synchronises.
 *
 *   spectrum_mul: out[z][i] = a[z or 0][i] * (conj ? conj(otf[z][i]) : otf[z][i]) on interleaved complex64, n complex values
 *                 per plane, D planes of otf and out (utils.py:501,700,715).  a_planes == D: a plane per depth (out == a, in
 *                 place, is allowed); a_planes == 1: one plane broadcast over the depths (the spectrum of the ratio image).
 *                 conj != 0 multiplies with the conjugate, so one stored transfer function serves both directions (utils.py:663).
 *                 otf is never written (out == otf is refused).
 *   project:      out[s][y][x] (+)= post(sum_z pre(p[s][z][(y + oy + sy) mod H][(x + ox + sx) mod W])), sy = ceil(H / 2),
 *                 sx = ceil(W / 2), for the Ho x Wo window at (oy, ox): batch_fftshift2d_real (the source index is the target index
 *                 plus the shift) fused with the relu and depth sum of utils.py:700 (pre = RELU, accumulate over depth chunks) or
 *                 the crop, depth sum and abs of utils.py:545-546 (post = ABS).  p: [N][D][H][W], out: [N][Ho][Wo].  The depths
 *                 are added in order z = 0 .. D-1 by the one thread that owns the pixel: bitwise reproducible, no atomics.
 *                 relu keeps NaN, as torch's.
 *   ratio:        tmp = img / (est + 1e-8f) over n elements (utils.py:701); *flag (device int, never cleared here) is set to 1
 *                 when an element of tmp is NaN or one of img is not finite -- the condition under which the reference, whose
 *                 estimate starts as 0 * img (utils.py:677), leaves its loop (utils.py:707).
 *   clamp:        in place min(max(tmp, 0), *median * mult), NaN kept (torch.clamp_, utils.py:703), bound and count read from
 *                 device memory (the outputs of cwfa_select_nonzero_f32); nothing is written when *count == 0 (utils.py:702).
 *   update:       obj_pad[z][po + y][po + x] *= b[z][(po + y + s) mod F][(po + x + s) mod F], s = ceil(F / 2), for the interior
 *                 obj x obj window of D zero-padded F x F planes (utils.py:694,715: pad, product with the shifted back projection,
 *                 crop).  Only the window of either tensor is touched: the border of obj_pad stays exactly 0. */
enum { CWFA_DECONV_PRE_NONE = 0, CWFA_DECONV_PRE_RELU = 1 };
enum { CWFA_DECONV_POST_NONE = 0, CWFA_DECONV_POST_ABS = 1 };
int cwfa_deconv_spectrum_mul_c64(const float* a, const float* otf, float* out, int D, int64_t n, int a_planes, int conj, void* stream);
int cwfa_deconv_project_f32(const float* p, float* out, int N, int D, int H, int W, int Ho, int Wo, int oy, int ox, int pre, int post,
                            int accumulate, void* stream);
int cwfa_deconv_ratio_f32(const float* img, const float* est, float* tmp, int* flag, int64_t n, void* stream);
int cwfa_deconv_clamp_f32(float* tmp, int64_t n, const float* median, const int64_t* count, float mult, void* stream);
int cwfa_deconv_update_f32(float* obj_pad, const float* b, int D, int F, int obj, int po, void* stream);

/* Vector extrapolation (Biggs & Andrews, Appl. Opt. 36, 1997) of the iteration above, a convergence trace for either loop
 * (DESIGN.md section 20).  The padded object holds the prediction y_k the FFTs read; the Richardson-Lucy iterates x_k, x_{k+1} and
 * the step g_k = x_{k+1} - y_k live in window-sized buffers [D][obj][obj].  Same conventions as the block above; the sums are
 * float64 block partials in a slab, added in a fixed order: no atomics, bitwise repeatable.  Nothing is allocated, nothing
 * synchronises, the host reads nothing back.
 *
 *   update_accel: in place of update, per depth chunk: x_new = obj_pad window * shifted(b) (the same single fp32 product), g =
 *                 x_new - obj_pad window; obj_pad and b are only read.  g_prev is read before g is written: g == g_prev, in place,
 *                 is allowed.  x_new and g share no buffer with an input or each other.  Slab row (depth within the chunk, block)
 *                 += (sum g * g_prev, sum g_prev^2) over the block's elements, products exact in float64; the rows of the chunks of
 *                 one iteration coincide and are added to in launch order.  slab: 2 * slab_rows doubles, 8-byte aligned, zero
 *                 before the first chunk of an iteration; slab_rows >= D * ceil(units / CWFA_DECONV_ACCEL_UNITS), units = obj * obj
 *                 window elements (obj * obj / 4 sixteen-byte groups where F, obj, po and ceil(F / 2) are multiples of 4 and every
 *                 pointer is 16-byte aligned): D * ceil(obj * obj / CWFA_DECONV_ACCEL_UNITS) rows always suffice.
 *   alpha:        one block: *alpha = float(clamp(sum of column 0 / sum of column 1, 0, alpha_max)) over `rows` rows of the slab, 0
 *                 when the quotient is not finite (zero denominator: no previous step; NaN).  The rows are zeroed for the next
 *                 iteration.  alpha_max in [0, 1).
 *   predict:      obj_pad window = max(x_new + *alpha * (x_new - x_prev), 0) over all D depths, alpha read from device memory;
 *                 difference, product and sum are three separately rounded fp32 operations, NaN is kept.  Only the window of
 *                 obj_pad is written: its border stays exactly 0.
 *   poisson_nll:  trace[index] = sum over n elements of est - img * log(est + 1e-8), terms and sums in float64: one pass, at most
 *                 CWFA_DECONV_NLL_WORKSPACE_BYTES / 8 block partials in `workspace` (that many device bytes, 8-byte aligned, no
 *                 clearing needed), then one block adds them in ascending order.  0 <= index < trace_len.  n == 0 writes 0. */
#define CWFA_DECONV_ACCEL_UNITS 1024
#define CWFA_DECONV_NLL_WORKSPACE_BYTES 8192
int cwfa_deconv_update_accel_f32(const float* obj_pad, const float* b, const float* g_prev, float* x_new, float* g, double* slab,
                                 int64_t slab_rows, int D, int F, int obj, int po, void* stream);
int cwfa_deconv_alpha_f64(double* slab, int64_t rows, double alpha_max, float* alpha, void* stream);
int cwfa_deconv_predict_f32(float* obj_pad, const float* x_new, const float* x_prev, const float* alpha, int D, int F, int obj, int po,
                            void* stream);
int cwfa_deconv_poisson_nll_f32(const float* img, const float* est, int64_t n, double* trace, int64_t index, int64_t trace_len,
                                void* workspace, void* stream);

/* MAP Richardson-Lucy: the two updates above under an independent Gaussian prior N(mu, 1 / w) per voxel.
 * With a the plain update (window * shifted(b)), the new value is M(a, mu, w), the x > 0 that maximises
 * -x + a log x - w / 2 (x - mu)^2:
 *     c = 1 - w * mu,  r = sqrt(max(c * c + 4 * (w * a), 0)),  x = c > 0 ? 2a / (c + r) : (r - c) / (2w)
 * in fp32, one rounding per operation, square root and division correctly rounded.  w == 0 returns a's bits (a below 2^127);
 * a == 0 with c <= 0 returns mu - 1 / w; the maximum with 0 only acts for a < 0 and keeps NaN.  The caller keeps w and w * |mu|
 * small enough that c * c, 4 * w * a and 2 * w stay finite.  mu, w: [D][obj][obj] contiguous like g / x_new, only read, no buffer
 * shared with an output.  Same conventions as the blocks above.
 *
 *   update_map:        update's walk, in place: obj_pad window = M(obj_pad window * shifted(b), mu, w).
 *   update_accel_map:  update_accel's walk and slab: x_new = M(obj_pad window * shifted(b), mu, w), g = x_new - obj_pad window.
 *   Both, when pen_slab is not NULL: pen_slab row (depth within the chunk, block) += the block's sum of
 *                      0.5 * w * (y - mu)^2 over the window y as read, every operation in float64; the rows of the chunks of one
 *                      iteration coincide and are added to in launch order.  pen_slab: pen_rows doubles, 8-byte aligned, zero
 *                      before the first chunk; pen_rows >= D * ceil(units / CWFA_DECONV_UPDATE_UNITS) for update_map and
 *                      D * ceil(units / CWFA_DECONV_ACCEL_UNITS) for update_accel_map, units as for update_accel:
 *                      D * ceil(obj * obj / CWFA_DECONV_UPDATE_UNITS) rows always suffice for either.
 *   penalty:           one block: trace[index] += the sum of `rows` rows of pen_slab, each thread adding its rows in ascending
 *                      order, then the block sum (one fixed order), onto what poisson_nll wrote there; the rows are zeroed. */
#define CWFA_DECONV_UPDATE_UNITS 256
int cwfa_deconv_update_map_f32(float* obj_pad, const float* b, const float* mu, const float* w, double* pen_slab, int64_t pen_rows, int D,
                               int F, int obj, int po, void* stream);
int cwfa_deconv_update_accel_map_f32(const float* obj_pad, const float* b, const float* g_prev, const float* mu, const float* w,
                                     float* x_new, float* g, double* slab, int64_t slab_rows, double* pen_slab, int64_t pen_rows, int D,
                                     int F, int obj, int po, void* stream);
int cwfa_deconv_penalty_f64(double* pen_slab, int64_t rows, double* trace, int64_t index, int64_t trace_len, void* stream);

/* Neuron detection behind a reconstructed time series: the producer of the `coords` / `boxes` that roi_means,
 * corr_coeff_3D and the ROI posterior moments take (the reference reads them from a hand-annotated file, CWFA.py:223-238).  Every
 * floating-point operation is rounded separately.  Arguments are checked before any device work.
 *
 *   activity_update: adds the chunk x [T, m] (fp32, time stride x_ss >= m elements) to a per-voxel state of m voxels, 28 bytes each:
 *                    x0 (fp32, the first sample ever seen), s1 / s2 (float64 sums of d = (double)x - (double)x0 and of d * d, added in
 *                    time order), vmax / vmin (fp32; NaN propagates, as in torch.amax / amin).  first != 0: the state is initialised
 *                    from the chunk's first volume (T >= 1) and not read.  The additions per voxel happen in the same order however
 *                    the series is cut into chunks, and they are those of stack_mean_std.  One thread owns a group of voxels and walks
 *                    the chunk's time axis: no atomics; 16-byte accesses where m, x_ss and every pointer allow, element by element
 *                    otherwise.  T == 0 (first == 0) or m == 0: no launch.
 *   activity_finish: mean[m], std[m] (fp32) from the state of N samples by stack_mean_std's formulae -- bit for bit its results on the
 *                    concatenated series; unbiased std, N = 1 gives NaN -- and score[m] from the fp32 maps, each operation rounded to
 *                    fp32: ACTIVITY_STD: std; ACTIVITY_RANGE: vmax - vmin; ACTIVITY_PEAK: vmax - mean; ACTIVITY_SNR: (vmax - mean) / std,
 *                    0 where std == 0.
 *   local_maxima:    the 3-D local maxima of score [D, H, W] under the total order
 *                        key(v) = ord(S[v]) << 32 | (0xFFFFFFFF - lin(v)),
 *                    ord the order-preserving unsigned image of the fp32 bits of S[v] + 0.0f (-0 and +0 are one value; NaN -> 0), lin
 *                    the linear index (D * H * W <= 2^32, CWFA_E_SHAPE otherwise).  v is a peak iff S[v] is not NaN, S[v] >= thr, v
 *                    lies at least (mz, my, mx) voxels from every face, and key(v) is the maximum of the keys over the box |z'| <= dz,
 *                    |y'| <= dy, |x'| <= dx around it, clipped by the volume (voxels inside the margin still suppress their
 *                    neighbours).  A plateau yields the voxel of lowest linear index in each window; two peaks differ by more than the
 *                    half-width on at least one axis.  Half-widths 0 .. CWFA_NMAX_MAX_DIST, CWFA_E_SHAPE beyond.  Two launches: the
 *                    in-plane maximum of the keys from a haloed tile in the LDS into `workspace` (8 * D * H * W device bytes, 8-byte
 *                    aligned), then a walk along z per pixel.  Peaks are appended to `out` (`capacity` entries of 8 bytes: the fp32
 *                    score's bits, then the 32-bit linear index) through the device counter *count (int64, cleared by the call),
 *                    which keeps counting past `capacity`: *count is the number of peaks, min(*count, capacity) entries are
 *                    written, in no particular order -- order them by key.  Nothing synchronises: the caller reads *count. */
#define CWFA_NMAX_MAX_DIST 16
enum { CWFA_ACTIVITY_STD = 0, CWFA_ACTIVITY_RANGE = 1, CWFA_ACTIVITY_PEAK = 2, CWFA_ACTIVITY_SNR = 3 };
int cwfa_activity_update_f32(const float* x, float* x0, double* s1, double* s2, float* vmax, float* vmin, int T, int64_t m, int64_t x_ss,
                             int first, void* stream);
int cwfa_activity_finish_f32(const float* x0, const double* s1, const double* s2, const float* vmax, const float* vmin, int64_t N, int kind,
                             float* mean, float* std, float* score, int64_t m, void* stream);
int cwfa_local_maxima_f32(const float* score, int D, int H, int W, float thr, int dz, int dy, int dx, int mz, int my, int mx,
                          void* workspace, void* out, int64_t capacity, int64_t* count, void* stream);

/* ---- streaming local correlation: a neighbour-aware score for the detector above.  A neuron's voxels move
 * together, noise does not: the score of a voxel is the mean Pearson correlation of its series with its neighbours'.
 *
 * `neighbours` selects the offsets (dz, dy, dx): CORR_6 the faces, CORR_8 the in-plane ring (dz = 0), CORR_26 the cube.  The forward
 * offsets o_0 .. o_{K-1} are the lexicographically positive half in lexicographic order, K = 3, 4, 13: (0,0,1), then the dz = 0,
 * dy = 1 ones, then the dz = 1 ones.
 *
 *   activity_update_corr: everything activity_update does on volumes [D, H, W] (m = D * H * W; x0, s1, s2, vmax, vmin come out bit
 *                    for bit what that entry point writes), and in the same read of the chunk
 *                        cc[k][i] += d_i(t) * d_j(t),  j = i + o_k,  d = (double)x - (double)x0,
 *                    in time order from 0.0, over the samples after the first; cc is float64 [K, D, H, W], 8 K bytes per voxel.
 *                    The neighbour is taken by coordinates; where it is outside the volume cc[k][i] is 0.0.  d_j is formed from x_j
 *                    and x0_j exactly as the owner of j forms it (in the first chunk x0 is read from x[0]).  Every thread writes its
 *                    own voxels' state only: no atomics, any chunking gives the same bits.  16-byte accesses where W % 4 == 0,
 *                    x_ss % 4 == 0 and every pointer allow, element by element otherwise.  T == 0 (first == 0) or m == 0: no launch.
 *   activity_corr_finish: score[m] (fp32) from the state of N samples, in float64 per pair (i, j):
 *                        v_i = max(s2_i - s1_i * s1_i / N, 0),  cov = c - s1_i * s1_j / N,  den = sqrt(v_i * v_j),
 *                        r = den > 0 ? cov / den : 0            (c: cc[k] at the lower voxel of the pair)
 *                    score_i = (float)(sum of r / n_i) over the n_i in-volume offsets of the whole neighbourhood in lexicographic
 *                    order, 0 where n_i == 0.  A constant voxel, NaN or inf in a series and N == 1 give r = 0: never NaN.  The
 *                    state is only read. */
enum { CWFA_CORR_6 = 6, CWFA_CORR_8 = 8, CWFA_CORR_26 = 26 };
int cwfa_activity_update_corr_f32(const float* x, float* x0, double* s1, double* s2, float* vmax, float* vmin, double* cc, int T, int D,
                                  int H, int W, int64_t x_ss, int neighbours, int first, void* stream);
int cwfa_activity_corr_finish_f32(const double* s1, const double* s2, const double* cc, int64_t N, int D, int H, int W, int neighbours,
                                  float* score, void* stream);

/* ---- stimulus and seed regression maps: the per-voxel linear regression of the streamed series against K known
 * time courses r[t][0 .. K) (float64 rows, 1 <= K <= CWFA_REGRESS_MAX_K; the intercept is implicit), from sums kept beside the state
 * of activity_update.  Every float64 operation is rounded separately, in the order written here.
 *
 *   activity_update_regress: everything activity_update does (x0, s1, s2, vmax, vmin come out bit for bit what that entry point
 *                    writes), and in the same read of the chunk  p[k][i] += d_i(t) * r[t][k],  d = (double)x - (double)x0,  in time
 *                    order from 0.0 over the samples after the first (d of the first is exactly 0); p is float64 [K, m], rows the
 *                    chunk's [T, K] on the device.  K <= 8: one launch; beyond, a second launch over x adds the regressors from the
 *                    ninth on and writes p only.  16-byte accesses where m % 4 == 0, x_ss % 4 == 0 and every pointer allow, element
 *                    by element otherwise.  T == 0 (first == 0) or m == 0: no launch.
 *   regress_rows:    Sr[k] += r[t][k], Srr[k][l] += r[t][k] * r[t][l] (float64 [K], [K, K]) and *count += T over the chunk's rows in
 *                    time order -- over all samples, the first included; first != 0 starts them from 0.  One thread per (k, l).
 *   regress_design:  from the sums of N samples, by one thread:  G[k][l] = Srr[k][l] - Sr[k] * Sr[l] / N;  gdiag[k] = G[k][k];
 *                    G = L L' (Cholesky, row by row: pivot s = G[j][j] - L[j][0]^2 - .. - L[j][j-1]^2 subtracted in that order,
 *                    L[j][j] = sqrt(s), L[i][j] = (G[i][j] - L[i][0] L[j][0] - ..) / L[j][j]);  Linv column by column
 *                    (Linv[c][c] = 1 / L[c][c], Linv[i][c] = (0 - L[i][c] Linv[c][c] - .. - L[i][i-1] Linv[i-1][c]) / L[i][i]);
 *                    ginv[k][l] = Linv[q][k] * Linv[q][l] added from 0.0 over q = max(k, l) .. K - 1.
 *                    status[0] (int32 pair on the device, written always): 0, or REGRESS_COLLINEAR when a pivot is not above
 *                    rcond * G[j][j] or G[j][j] is not above rcond * Srr[j][j] (a constant regressor), REGRESS_NONFINITE when
 *                    an entry of Sr / Srr is NaN or inf, REGRESS_COUNT when *count != N; status[1]: the regressor.  On a non-zero
 *                    status gdiag and ginv are 0.
 *   regress_finish:  per voxel, with a = s1, vx = s2 - a * a / N, c[k] = p[k] - a * Sr[k] / N:
 *                        corr[k] = c[k] / sqrt(vx * gdiag[k]);   beta[k] = ginv[k][0] * c[0] + .. added from 0.0 in this order;
 *                        rss = max(vx - (c[0] * beta[0] + ..), 0);   t[k] = beta[k] / sqrt(rss / (N - K - 1) * ginv[k][k]), 0 where
 *                        that root is 0;   r2 = 1 - rss / vx
 *                    rounded to fp32 at the store; every map is 0 where vx is not > 0 or s1, s2 or a p[k] is not finite.  `want`
 *                    is a mask of REGRESS_CORR .. REGRESS_R2: only those are computed and stored, the other pointers may be null.
 *                    t needs N - K - 1 >= 1 (CWFA_E_SHAPE).  The state is only read.  m == 0: no launch. */
#define CWFA_REGRESS_MAX_K 16
enum { CWFA_REGRESS_CORR = 1, CWFA_REGRESS_BETA = 2, CWFA_REGRESS_T = 4, CWFA_REGRESS_R2 = 8 };
enum { CWFA_REGRESS_COLLINEAR = 1, CWFA_REGRESS_NONFINITE = 2, CWFA_REGRESS_COUNT = 3 };
int cwfa_activity_update_regress_f32(const float* x, const double* rows, float* x0, double* s1, double* s2, float* vmax, float* vmin,
                                     double* p, int T, int K, int64_t m, int64_t x_ss, int first, void* stream);
int cwfa_regress_rows_f64(const double* rows, int T, int K, double* Sr, double* Srr, int64_t* count, int first, void* stream);
int cwfa_regress_design_f64(const double* Sr, const double* Srr, const int64_t* count, int64_t N, int K, double rcond, double* gdiag,
                            double* ginv, int* status, void* stream);
int cwfa_regress_finish_f32(const double* s1, const double* s2, const double* p, const double* Sr, const double* gdiag,
                            const double* ginv, int64_t N, int K, int64_t m, int want, float* corr, float* beta, float* t, float* r2,
                            void* stream);

/* ---- shot noise: a Poisson draw per element, in one launch, nothing read back.
 *   out[s][e] = fl32(fl32(k) * post[s]),   k ~ Poisson(rate),   rate = fl32(lam[s * lam_ss + e] * pre[s])
 * for s < N, e < n.  pre / post: nullable DEVICE float [N], NULL means 1.  lam_ss = 0: all N samples draw from one rate plane;
 * out == lam (in place) is allowed when lam_ss == out_ss: an element reads only its own rate, before it writes.  Strides in
 * elements, >= n (out_ss > n leaves the gap untouched).  n <= 2^52, CWFA_E_SHAPE beyond.
 * Counter convention -- part of the interface, and NOT that of cwfa_rand_uniform_f32 above (which packs four elements into a
 * block): element e of sample s, round t, uses the Philox4x32-10 block with counter
 *   (e & 0xffffffff, (e >> 32) | (t << 20), sample_offset + s, stream_id)   under the key (seed & 0xffffffff, seed >> 32),
 * one block per element and round, so a draw depends on nothing but (seed, stream_id, sample_offset + s, e) and its rate: samples
 * [0, N) equal [0, k) followed by [k, N) under sample_offset + k, bit for bit.  A word r becomes u = (r + 0.5) * 2^-32 in float64
 * (exact, strictly inside (0, 1)); every comparison of the draw is evaluated in float64:
 *   rate < 10    inversion by sequential search on word 0 of round 0: k = 0, p = F = exp(-rate); while u > F and k < 80:
 *                k += 1, p *= rate / k, F += p.  Probabilities below 2^-33 are unreachable.
 *   rate >= 10   Hoermann's PTRS with b = 0.931 + 2.53 sqrt(rate), a = -0.059 + 0.02483 b, 1/alpha = 1.1239 + 1.1328 / (b - 3.4),
 *                v_r = 0.9277 - 3.6224 / (b - 2); attempt j takes (U, V) from words (2 (j & 1), 2 (j & 1) + 1) of round j >> 1.
 *                Bounded: after 32 rounds (64 attempts) k = rint(rate).
 *   rate = 0 gives 0; a rate that is negative, NaN or above 2^30 gives NaN in out.  fl32(k) is exact only below 2^24. */
int cwfa_rand_poisson_f32(float* out, const float* lam, int N, int64_t n, int64_t lam_ss, int64_t out_ss, const float* pre,
                          const float* post, uint64_t seed, uint32_t stream_id, uint32_t sample_offset, void* stream);

/* ---- sparse-activity extraction: a robust rank-1 background L[t,p] = a[t] * b[p] of a frame stack and the
 * thresholded positive residual S = relu(x - L - tau).  x: [T, P], `dtype` 0 = fp32, 1 = fp16, frame_stride >= P elements between
 * frames (a band of rows of every frame is a valid argument).  Inputs are assumed finite.  Arguments are checked before any device
 * work; nothing is allocated, nothing synchronises.  T == 0 or P == 0: no launch, CWFA_OK (frame_dots: P == 0, and sums that are
 * overwritten are cleared).
 *
 *   temporal_select:  out[k * P + p] (fp32) = the ranks[k]-th smallest (from 0) of the T values v[t] of pixel p; `ranks` is a HOST
 *                     array of K in 1 .. 4 entries in [0, T), duplicates allowed.  a == b == NULL: v = x (fp16 widened, exactly);
 *                     both given (device fp32 [T] and [P]): v = fl32(x - fl32(a[t] * b[p])), formed on load.  The result is an
 *                     element of v, bit for bit, under the order of local_maxima: the unsigned image of the fp32 bits of v + 0.0f
 *                     (-0 and +0 are one value, returned as +0).  Found by bisection of the key bits from the top, one count of
 *                     the keys per bit for all K ranks.  form 1, one read of the stack: a workgroup keeps the T keys of a tile of
 *                     64 pixels in the LDS (32-bit keys; 16-bit keys for fp16 without a background), its waves split the frames;
 *                     T <= temporal_select_lds_frames, CWFA_E_SHAPE beyond.  form 2, streaming: a thread per pixel counts from
 *                     memory, one sweep per key bit, any T.  form 0: form 1 where T fits, else form 2.  The forms agree bit for bit.
 *   temporal_select_lds_frames: host only: the largest T of form 1 for this dtype with (transformed != 0) or without a background.
 *   frame_dots:       sums[t] = sum_p x[t,p] * b[p] for t < T and sums[T] = sum_p b[p]^2, float64, every product formed in float64
 *                     (exact for fp32 factors).  Block partials go to `ws` (frame_dots_workspace_bytes(T, P) device bytes, 8-byte
 *                     aligned, no clearing needed) and are added in a fixed order: no atomics, bitwise repeatable.  accumulate = 1
 *                     adds to the T + 1 sums (bands of rows add up), 0 overwrites.  sums, ws: 8-byte aligned, CWFA_E_ALIGN otherwise.
 *   sparse_residual:  r = fl32(fl32(x - fl32(a[t] * b[p])) - tau[p]) (tau == NULL: without the last subtraction), S = r > 0 ? r : 0.
 *                     pair = 0: out fp32 [T, P]; out == x is allowed for an fp32 stack with frame_stride == P.  pair = 1: out fp32
 *                     [T, P, 2], channel 0 = x widened, channel 1 = S, written in the same pass.  16-byte accesses (8-byte loads of
 *                     fp16) where P, the stride and every base allow, element by element otherwise. */
int cwfa_temporal_select(const void* x, int dtype, int T, int64_t P, int64_t frame_stride, const float* a, const float* b,
                         const int* ranks, int K, float* out, int form, void* stream);
int cwfa_temporal_select_lds_frames(int dtype, int transformed);
int64_t cwfa_frame_dots_workspace_bytes(int T, int64_t P);
int cwfa_frame_dots(const void* x, int dtype, int T, int64_t P, int64_t frame_stride, const float* b, double* sums, void* ws,
                    int accumulate, void* stream);
int cwfa_sparse_residual(const void* x, int dtype, int T, int64_t P, int64_t frame_stride, const float* a, const float* b,
                         const float* tau, float* out, int pair, void* stream);

/* ---- rigid frame registration: phase correlation of the frames of a stack against a template, an integer
 * peak in a bounded window with parabolic sub-pixel refinement, resampling.  The transforms between these passes are rocFFT's.
 * Real stacks: [N, H, W], `dtype` 0 = fp32, 1 = fp16, frame_stride >= H * W elements between frames; H * W < 2^31.  Arguments are
 * checked before any device work; nothing is allocated, nothing synchronises, nothing is read back.  An empty problem: no launch,
 * CWFA_OK.
 *
 *   reg_window:     out[n,y,x] (fp32, contiguous) = fl32(float(x[n,y,x]) * fl32(wy[y] * wx[x])), wy [H] and wx [W] device fp32.
 *                   One read and one write; 16-byte accesses (8-byte loads of fp16) where W, the stride and the bases allow.
 *   reg_whiten_c64: F [N, bins] and out [N, bins] interleaved complex64, out == F allowed.  u = z / (|z| + eps) with
 *                   |z| = sqrtf(fl32(fl32(re re) + fl32(im im))) and two divisions; Wt == NULL: out = u; else Wt [bins] complex64 and
 *                   out = u * Wt (four products, a difference, a sum, each rounded).  A thread owns a bin and walks the frames.
 *                   eps >= 0, finite.  All three 8-byte aligned, CWFA_E_ALIGN otherwise.
 *   reg_peak_f32:   one workgroup per frame of the correlation maps c [N, H, W] fp32.  Window index i, row-major over
 *                   sy in [-my, my], sx in [-mx, mx], reads c at (sy mod H, sx mod W); the maximum of
 *                   key = ord(c + 0.0f) << 32 | (0xFFFFFFFF - i) under the order of local_maxima (NaN: ord 0; ties go to the lowest
 *                   index) is found without atomics.  2 my + 1 <= H and 2 mx + 1 <= W, CWFA_E_SHAPE otherwise.  subpixel = 1: per
 *                   axis, from the peak and its two neighbours modulo H / W, in float64: den = (c- - 2 c0) + c+,
 *                   d = (0.5 (c- - c+)) / den where den < 0 and d is finite, else 0, clamped to [-0.5, 0.5];
 *                   shifts[n] = (float)((double)peak + d).  Writes shifts fp32 [N, 2] (dy, dx), ipeak int32 [N, 2], peak fp32 [N] (the
 *                   map's value at the integer peak).  A window without a finite value: shift (0, 0), ipeak (0, 0), peak NaN.
 *                   shifts and ipeak 8-byte aligned, CWFA_E_ALIGN otherwise.
 *   reg_shift:      out[n,y,x] = sum of w * in[n, y + iy + r, x + ix + c] over the taps (r, c) = (0,0), (0,1), (1,0), (1,1) in that
 *                   order, (dy, dx) = shifts[n] read on the device, iy = floorf(dy), fy = fl32(dy - iy),
 *                   w = fl32((fl32(1 - fy), fy)[r] * (fl32(1 - fx), fx)[c]), every product and sum rounded to fp32.  A tap of weight
 *                   exactly 0 is neither read nor added: an integer shift copies the source bits.  A tap outside the frame reads
 *                   `fill`; a non-finite shift fills the frame.  mode 0 bilinear, 1 nearest (rintf of the shift first).  out
 *                   [N, H, W] contiguous of the input's dtype (fp16: round to nearest even of the fp32 sum), out != in.  A thread
 *                   writes four consecutive fp32 pixels (eight of fp16: 16 bytes; four of fp16 next) where W and out's base allow, one
 *                   otherwise.  shifts 8-byte aligned, CWFA_E_ALIGN otherwise. */
int cwfa_reg_window(const void* x, int dtype, int N, int H, int W, int64_t frame_stride, const float* wy, const float* wx,
                    float* out, void* stream);
int cwfa_reg_whiten_c64(const void* F, const void* Wt, int N, int64_t bins, float eps, void* out, void* stream);
int cwfa_reg_peak_f32(const float* c, int N, int H, int W, int64_t frame_stride, int my, int mx, int subpixel, float* shifts,
                      int* ipeak, float* peak, void* stream);
int cwfa_reg_shift(const void* in, int dtype, int N, int H, int W, int64_t frame_stride, const float* shifts, int mode, float fill,
                   void* out, void* stream);

/* ---- up-sampled-DFT refinement of the registration peak.  R: the whitened cross-power spectra, interleaved
 * complex64 [N, H, K], K = W / 2 + 1, frame_stride >= H K elements between frames; ipeak int32 [N, 2] as reg_peak_f32 writes it.
 * Everything is float64, every product and sum rounded separately; no atomics, nothing allocated, nothing synchronises; arguments are
 * checked before any device work; N == 0: no launch, CWFA_OK.  H, W >= 1 below 2^30 with H W, H u, W u < 2^31, u >= 1, 1 <= r < 2^14.
 *
 *   reg_upsample_c64:  C [N, U, U] (double), U = 2 r + 1: the trigonometric interpolant of irfft2(R) at y = py + (jy - r) / u,
 *                      x = px + (jx - r) / u.  With m_j = (p u + j - r) reduced modulo M = (W or H) u in integers:
 *                        Tx[kx, j] = w[kx] rootx[(kx m_j) mod (W u)],       w = 1 at kx = 0 and at kx = W / 2 (W even), else 2 (exact)
 *                        Ty[ky, j] = rooty[(s(ky) m_j) mod (H u)],          s(ky) = ky where 2 ky < H, else ky - H
 *                      the Nyquist column (kx = W / 2, W even) and row (ky = H / 2, H even) with imaginary part 0;
 *                        E[ky, jx] = sum over kx = 0 .. K - 1 in that order from (0, 0) of R[ky, kx] * Tx[kx, jx]
 *                                    (re = fl(fl(a c) - fl(b d)), im = fl(fl(a d) + fl(b c)), each added to its sum)
 *                        C[jy, jx] = fl(S * fl(1 / (H W))),  S = the sum over 8 segments of ceil(H / 8) rows, in order from 0.0, of
 *                                    the segment's sum over ky, in order from 0.0, of fl(fl(Ty.re E.re) - fl(Ty.im E.im)).
 *                      rootx [W u], rooty [H u]: DEVICE interleaved doubles, root[k] = exp(2 pi i k / M), the caller's tables,
 *                      16-byte aligned.  ws: reg_upsample_workspace_bytes(N, H, W, r) DEVICE bytes, 16-byte aligned (Tx, Ty and E,
 *                      16 N U (K + 2 H) bytes; nothing is written behind them).  R, ipeak, C 8-byte aligned, CWFA_E_ALIGN otherwise.
 *                      reg_upsample_workspace_bytes (host only) returns -1 for sizes the entry point refuses.
 *   reg_fine_peak_f64: one workgroup per frame of C [N, U, U], U odd >= 3: the maximum under the order of reg_peak_f32 widened to
 *                      64 bits (the image of the bits of c + 0.0, NaN below everything, ties to the lowest row-major index), found
 *                      without atomics; per axis, where the maximum is not on the border of the grid along it, the parabola of
 *                      reg_peak_f32 through it and its two fine neighbours (d in fine steps), else d = 0;
 *                      shifts[n] = (float)((double)p + ((double)(j - r) + d) / (double)u), peak[n] = (float)C at the maximum.  A map
 *                      without a finite value: shifts = the integer peak, peak NaN.  keep = 1: shifts and peak hold reg_peak_f32's
 *                      results and a frame whose peak is NaN there is left as it is (its map is not read); keep = 0: never read. */
int64_t cwfa_reg_upsample_workspace_bytes(int N, int H, int W, int r);
int cwfa_reg_upsample_c64(const void* R, int N, int H, int W, int64_t frame_stride, const int* ipeak, int u, int r, const double* rootx,
                          const double* rooty, double* C, void* ws, void* stream);
int cwfa_reg_fine_peak_f64(const double* C, const int* ipeak, int N, int U, int u, int keep, float* shifts, float* peak, void* stream);

/* ---- per-lenslet registration with an axial-motion fit.  A frame [H, W] holds L views, 1 <= L <= 254; centers is
 * a HOST int32 [L][2] table of (row, column), every entry inside +-2^29; it is checked and travels in the kernel arguments.  View i is
 * the box of rows cy_i - ph / 2 .. cy_i - ph / 2 + ph - 1 and the matching columns, ph, pw >= 1, ph pw < 2^31; it may leave the
 * frame.  Stacks as above (dtype 0 = fp32, 1 = fp16, frame_stride >= H W, H, W >= 1).  Arguments are checked before any device work;
 * nothing is allocated, nothing synchronises, no atomics; N == 0: no launch, CWFA_OK.  Every floating-point operation is rounded
 * separately.
 *
 *   reg_window_views:  out [N, L, ph, pw] fp32 contiguous = fl32(float(x[n, cy - ph/2 + y, cx - pw/2 + x]) * fl32(wy[y] * wx[x])), a
 *                      pixel outside the frame read as 0.0f; wy [ph], wx [pw] device fp32.  One read of the views' pixels, one write;
 *                      a thread owns four pixels of a view's row (16-byte stores) where pw % 4 == 0 and out is 16-byte aligned, one
 *                      otherwise, and reads them in one load of element alignment inside the frame.
 *   reg_label_map:     labels [H, W] device bytes: the index of the view whose box holds the pixel; among several the smallest integer
 *                      squared distance to the centre, ties to the lowest index; L where none does.
 *   reg_fit_views_f64: per frame n from shifts [N, L, 2] fp32, peak [N, L] fp32 and directions g [L, 2] float64 (all device), one
 *                      thread per frame, float64, sums over i = 0 .. L - 1 in order from 0.0 skipping views of weight 0:
 *                      w_i = 1 where peak is finite and >= min_peak, else 0; m = sum w; for m >= 1: gm = (sum w g) / m,
 *                      sm = (sum w s) / m, q = sum w (ey ey + ex ex) with e = g_i - gm, a = q > 0 ? (sum w (ey ty + ex tx)) / q : 0
 *                      with t = s_i - sm, d = sm - a gm.  Then r_i = max(|s_iy - (d_y + a g_iy)|, |s_ix - (d_x + a g_ix)|) and
 *                      w_i = 0 where r_i > reject; if a weight is left the fit is repeated, if none is the first fit and weights
 *                      stand.  m == 0: d = 0, a = 0.  params [N, 3] float64 = (d_y, d_x, a); inlier [N, L] bytes = the final w;
 *                      table [N, L + 1, 2] fp32: row L = (float)d; model 0 (axial): row i = (float)(d + a g_i); model 1 (free): row i
 *                      = s_i where inlier, the axial value where not.  min_peak, reject >= 0 (reject may be +inf), CWFA_E_INVAL
 *                      otherwise (NaN included).  directions, params, table 8-byte aligned, CWFA_E_ALIGN otherwise.
 *   reg_shift_labeled: reg_shift with (dy, dx) = table[n, min(labels[y,x], L)] (table [N, L + 1, 2] fp32, labels [H, W] bytes, both
 *                      device): the same taps, weights, order, fill and store forms, bit for bit; the source is the whole frame.
 *                      A thread resamples its group of pixels once per label in the group (once where the labels agree) and keeps, of
 *                      each pass, the pixels that carry the label: every pixel comes from its own taps by the same code.
 *                      out != in; table 8-byte aligned, CWFA_E_ALIGN otherwise. */
int cwfa_reg_window_views(const void* x, int dtype, int N, int H, int W, int64_t frame_stride, const int32_t* centers, int L, int ph,
                          int pw, const float* wy, const float* wx, float* out, void* stream);
int cwfa_reg_label_map(const int32_t* centers, int L, int ph, int pw, int H, int W, uint8_t* labels, void* stream);
int cwfa_reg_fit_views_f64(const float* shifts, const float* peak, const double* directions, int N, int L, double min_peak, double reject,
                           int model, double* params, uint8_t* inlier, float* table, void* stream);
int cwfa_reg_shift_labeled(const void* in, int dtype, int N, int H, int W, int64_t frame_stride, const float* table, const uint8_t* labels,
                           int L, int mode, float fill, void* out, void* stream);

/* ---- rigid registration of reconstructed volumes: the passes of section 26 for stacks of volumes.  Volumes are
 * fp32 [N, D, H, W], every volume contiguous, vol_stride >= D * H * W elements between volumes; D, H, W < 2^30, D * H * W < 2^31; all
 * offsets are 64-bit (a stack may exceed 2^31 elements).  The spectra between the passes are whitened by reg_whiten_c64 with
 * bins = D * H * (W / 2 + 1).  Arguments are checked before any device work; nothing is allocated, nothing synchronises, no atomics,
 * nothing is read back; N == 0 (or an empty volume): no launch, CWFA_OK.  The grids stay inside the hardware limits for any N: the
 * kernels walk the volumes.  Every pointer 4-byte aligned, CWFA_E_ALIGN otherwise.
 *
 *   reg_window3d_f32: out[n,z,y,x] (contiguous) = fl32(x[n,z,y,x] * fl32(fl32(wz[z] * wy[y]) * wx[x])), wz [D], wy [H], wx [W] device
 *                     fp32.  One read and one write; 16-byte accesses where W, the stride and the bases allow, element by element
 *                     otherwise.  D = 1 with wz = {1}: the bits of reg_window.  out != x.
 *   reg_peak3d_f32:   one workgroup per volume of the correlation maps c.  Window index i, row-major over sz in [-mz, mz],
 *                     sy in [-my, my], sx in [-mx, mx], reads c at the shifts modulo (D, H, W); the maximum of
 *                     key = ord(c + 0.0f) << 32 | (0xFFFFFFFF - i) under the order of reg_peak_f32, by wave shuffles and through the
 *                     LDS.  2 m + 1 <= the side on every axis, CWFA_E_SHAPE otherwise.  subpixel = 1: the float64 parabola of
 *                     reg_peak_f32 per axis (its guards, its clamp to +-0.5), from the peak's neighbours modulo the side.  Writes
 *                     shifts fp32 [N, 3] (dz, dy, dx), ipeak int32 [N, 3], peak fp32 [N].  A window without a finite value: shift 0,
 *                     ipeak 0, peak NaN.  D = 1, mz = 0: columns 1 and 2 and peak are the bits of reg_peak_f32.
 *   reg_shift3d_f32:  (dz, dy, dx) = shifts[n] (fp32 [N, 3]) read on the device; a non-finite component fills the volume with `fill`;
 *                     mode 1 (nearest) applies rintf to all three first.  iz = floorf(dz), fz = fl32(dz - iz),
 *                     wz = (fl32(1 - fz), fz); for r = 0, 1 with wz[r] != 0, p_r[y,x] is what reg_shift's rule gives for plane
 *                     z + iz + r under (dy, dx), a plane outside the volume holding `fill` everywhere;
 *                     out = fl32(wz[0] p_0), then + fl32(wz[1] p_1), each rounded; a plane of weight exactly 0 is neither read nor
 *                     added.  So an integer shift copies source bits, an integer dz gives reg_shift's bits on plane z + dz, and
 *                     D = 1, dz = 0 gives reg_shift's bits.  out [N, D, H, W] contiguous, out != in.  A thread writes four
 *                     consecutive voxels of a row in one 16-byte store where W and out's base allow, one voxel otherwise, and walks
 *                     up to 16 planes keeping p_1 as the next plane's p_0: a source plane is read once per 16 output planes. */
int cwfa_reg_window3d_f32(const float* x, int N, int D, int H, int W, int64_t vol_stride, const float* wz, const float* wy, const float* wx,
                          float* out, void* stream);
int cwfa_reg_peak3d_f32(const float* c, int N, int D, int H, int W, int64_t vol_stride, int mz, int my, int mx, int subpixel, float* shifts,
                        int* ipeak, float* peak, void* stream);
int cwfa_reg_shift3d_f32(const float* in, int N, int D, int H, int W, int64_t vol_stride, const float* shifts, int mode, float fill,
                         float* out, void* stream);

/* ---- piecewise-rigid registration of volumes: a volume is cut into gz x gy x gx blocks (B = gz gy gx <= 4096,
 * block b = (iz gy + iy) gx + ix), every block is registered by the passes above on the batch of N B blocks, the table of block shifts
 * is cleaned, interpolated between the block centres and the volume resampled once under a displacement per voxel.  Arguments are
 * checked before any device work (CWFA_E_INVAL / _SHAPE / _ALIGN as above), offsets are 64-bit, nothing is allocated or read back,
 * no atomics, N == 0 launches nothing, no grid axis grows with N.
 *   reg_window_blocks3d_f32: out[n,b,z,y,x] = fl32(x[n, oz+z, oy+y, ox+x] * fl32(fl32(wz[z] wy[y]) wx[x])), fp32 [N, B, bz, by, bx]
 *                     contiguous.  `origins`: a HOST int32 table, the gz origins of axis z, then gy of y, then gx of x, each checked
 *                     to keep the block inside the volume (0 <= o <= side - b) and carried to the kernel in its arguments.  One
 *                     read of each block, one write; 16-byte stores where bx and out's base allow, loads of element alignment.
 *   reg_field_fill:   shifts fp32 [N, B, 3], peak fp32 [N, B], base fp32 [N, 3] on the device; `max_dev`: three HOST doubles or null.
 *                     A node is an inlier when its peak is finite and >= min_peak, its components are finite and (max_dev given)
 *                     |s_c - base_c| <= max_dev[c], compared in float64.  field [N, B, 3]: an inlier's bits; for an outlier, per
 *                     component, the float64 mean of the inliers among its 26 grid neighbours (row-major over {-1,0,1}^3, z slowest,
 *                     status read from the input) rounded once to fp32, or base[n] where it has none.  inlier uint8 [N, B].
 *                     field != shifts.  One thread per node, bitwise repeatable.
 *   reg_warp3d_f32:   field fp32 [N, B, 3] and the six axis tables on the device (idx int32, t fp32, one entry per coordinate: the
 *                     node at or below and the fraction towards the next; an idx is clamped to the grid, and node idx + 1 is never
 *                     read where t == 0 or idx is the last node).  (dz, dy, dx) of a voxel: lerp(a, b, t) = a where t == 0, else
 *                     fl32(a + fl32(t fl32(b - a))), along x, then y, then z.  out[n,z,y,x] = reg_shift3d_f32's rule under that vector,
 *                     voxel by voxel: a field whose nodes are equal gives reg_shift3d_f32's bits.  out != in.  A thread writes four
 *                     consecutive voxels in one 16-byte store where W and out's base allow, one otherwise, and walks up to 16
 *                     planes, keeping the (y, x) interpolation of its two node planes. */
int cwfa_reg_window_blocks3d_f32(const float* x, int N, int D, int H, int W, int64_t vol_stride, const int32_t* origins, int gz, int gy, int gx,
                                 int bz, int by, int bx, const float* wz, const float* wy, const float* wx, float* out, void* stream);
int cwfa_reg_field_fill(const float* shifts, const float* peak, const float* base, int N, int gz, int gy, int gx, double min_peak,
                        const double* max_dev, float* field, unsigned char* inlier, void* stream);
int cwfa_reg_warp3d_f32(const float* in, int N, int D, int H, int W, int64_t vol_stride, const float* field, int gz, int gy, int gx,
                        const int32_t* idxz, const float* tz, const int32_t* idxy, const float* ty, const int32_t* idxx, const float* tx, int mode,
                        float fill, float* out, void* stream);

/* ---- rigid registration of volumes with a rotation about the optical axis: the block-shift table of section 32
 * is fitted by "rotation about z + 3-D shift" and the volume is resampled once under it.  A motion is five float64 numbers
 * (dz, dy, dx, c, s), c = cos, s = sin of the angle, and moves a volume as
 *   out(z, y, x) = in(z + dz, c0 + R ((y, x) - c0) + (dy, dx)),  R = [[c, -s], [s, c]] on (y, x),  c0 = (cy, cx);
 * c - 1 is always formed as cm1 = -(s s) / (1 + c); no trigonometric function is evaluated.  Arguments are checked before any device
 * work (CWFA_E_INVAL / _SHAPE / _ALIGN as above), offsets are 64-bit, nothing is allocated or read back, no atomics, N == 0 launches
 * nothing.  Every floating-point operation is rounded separately.
 *   reg_fit_rigid_f64: per volume n from shifts fp32 [N, B, 3], peak fp32 [N, B] and arms a float64 [B, 2] (block centre - c0, (y, x);
 *                     all device), 1 <= B <= 4096, one thread per volume, float64, sums over b = 0 .. B - 1 in order from 0.0
 *                     skipping blocks of weight 0: w_b = 1 where peak is finite and >= min_peak and the three components are finite;
 *                     m = sum w; for m >= 1: am = (sum w a) / m, sm = (sum w s) / m, e = a_b - am, f = e + (s_b,yx - sm_yx),
 *                     P = sum w (ey fy + ex fx), Q = sum w (ey fx - ex fy), r = sqrt(P P + Q Q); (c, s) = (P / r, Q / r) where r > 0,
 *                     P > 0 and both are finite, else (1, 0); dz = sm_z, dy = sm_y - (cm1 am_y - s am_x),
 *                     dx = sm_x - (s am_y + cm1 am_x).  Then r_b = max(|s_z - dz|, |s_y - (dy + (cm1 a_y - s a_x))|,
 *                     |s_x - (dx + (s a_y + cm1 a_x))|) and w_b = 0 where r_b > reject; if a weight is left the fit is repeated
 *                     once, if none is the first fit and weights stand.  m == 0: (0, 0, 0, 1, 0).  prior [N, 5] float64 or null: the
 *                     motion (dz', dy', dx', c', s') already applied to the measured volumes; the result is then the total motion,
 *                     C = c' c - s' s, S = s' c + c' s, h = sqrt(C C + S S), rotation (C / h, S / h),
 *                     dy = (dy + (cm1' dy - s' dx)) + dy', dx = (dx + (s' dy + cm1' dx)) + dx', dz = dz + dz'.  params [N, 5]
 *                     float64, inlier [N, B] bytes = the final w.  min_peak, reject >= 0 (reject may be +inf), CWFA_E_INVAL otherwise
 *                     (NaN included); arms, params, prior 8-byte aligned; params != prior.  Bitwise repeatable.
 *   reg_rigid3d_f32:  params [N, 5] float64 read on the device; cy, cx two finite host floats.  Per volume dzf, dyf, dxf, sf = the fp32
 *                     roundings of dz, dy, dx, s and cm1f = (float)cm1 (cm1 in float64); a c that is not finite or a non-finite one
 *                     of those five fills the volume with `fill`.  Per voxel py = fl32((float)y - cy), px = fl32((float)x - cx),
 *                     vy = fl32(dyf + fl32(fl32(cm1f py) - fl32(sf px))), vx = fl32(dxf + fl32(fl32(sf py) + fl32(cm1f px))) and
 *                     out[n,z,y,x] = reg_shift3d_f32's rule under (dzf, vy, vx), `fill` where vy or vx overflowed: (c, s) = (1, 0) gives reg_shift3d_f32's bits, an
 *                     integer shift without rotation copies source bits, (0, +-1) about the centre of a square plane is a quarter
 *                     turn of every plane, bit for bit.  out [N, D, H, W] contiguous, out != in.  A thread writes four consecutive
 *                     voxels of a row in one 16-byte store where W and out's base allow, one voxel otherwise, forms their (vy, vx)
 *                     once per volume and walks up to 16 planes keeping p_1 as the next plane's p_0. */
int cwfa_reg_fit_rigid_f64(const float* shifts, const float* peak, const double* arms, int N, int B, double min_peak, double reject,
                           const double* prior, double* params, uint8_t* inlier, void* stream);
int cwfa_reg_rigid3d_f32(const float* in, int N, int D, int H, int W, int64_t vol_stride, const double* params, float cy, float cx, int mode,
                         float fill, float* out, void* stream);

/* ---- neuron footprints: behind the detector, which voxels of a neuron's ROI box move with its centre once the
 * signal shared with the surroundings is taken out, and the traces weighted by that.  x: volumes [T, D, H, W] fp32, contiguous
 * volumes, t_stride >= D * H * W elements between them.  Box tables are HOST int32 [N][6] = {z0,z1,y0,y1,x0,x1}, half-open, inside the
 * volume and below 2^31 voxels each (as cwfa_roi_means_f32); they are checked and travel in the kernel arguments, any N.  The state is
 * ragged: offsets is HOST int64 [N + 1], offsets[0] = 0, offsets[n + 1] - offsets[n] = the volume of box n, V = offsets[N]; box n's
 * voxels lie at offsets[n] in the box's own (z, y, x) linear order, so overlapping boxes share nothing.  Arguments are checked before
 * any device work; nothing is allocated, nothing synchronises, no atomics.  N == 0 or T == 0: no launch, CWFA_OK.  Float64 arrays are
 * 8-byte aligned, CWFA_E_ALIGN otherwise.  Every floating-point operation is rounded separately.
 *
 *   roi_mark:          occ [D, H, W] (device bytes) = 1 inside any box, 0 elsewhere (the call clears the map; every writer stores 1).
 *   roi_weighted_sums: out[n][t] (double) = sum over box n of w[offsets[n] + i] * x[t, voxel i], each product exact in float64, added
 *                      by one wave in a fixed tree.  w == NULL: the plain sum (offsets is then not read).  An empty box gives 0.
 *   roi_shell_sums:    sums[n][t] (double) = the sum of x[t] over the voxels of outer[n] that are outside inner[n] and have occ == 0,
 *                      by one workgroup in a fixed tree; counts[n] (int32) = their number (written when T >= 1).
 *   footprint_update:  adds the chunk to the state x0 [V] (fp32), acc [4][V] (double: s1, s2, sc, su), ref [N][7] (double: c0, u0, e1,
 *                      e2, g1, g2, eg).  c, u: DEVICE double [N][T], the seed and neuropil traces of the chunk (u == NULL: without
 *                      neuropil; su, u0, g1, g2, eg are then written as 0.0 by the first chunk and kept).  With x0 the voxel's first
 *                      sample ever seen, c0 / u0 the traces' first values, d = (double)x - (double)x0, e = c - c0, g = u - u0:
 *                          s1 += d, s2 += d d, sc += d e, su += d g          e1 += e, e2 += e e, g1 += g, g2 += g g, eg += e g
 *                      in time order from 0.0, the first chunk (first != 0, T >= 1) skipping its own first volume: the state after
 *                      any chunking is bit for bit that of the whole series.  A thread owns a state voxel and walks the time axis.
 *   footprint_corr:    corr[V] (fp32) from the state of T samples, a thread per state voxel, in float64:
 *                          v_a = max(s2_a - s1_a s1_a / T, 0),  r_ab = den > 0 ? (s_ab - s1_a s1_b / T) / den : 0,  den = sqrt(v_a v_b)
 *                      for the pairs voxel-seed (ie), voxel-neuropil (ig), seed-neuropil (eg); neuropil != 0:
 *                          q = (1 - r_ig r_ig)(1 - r_eg r_eg),  r = q > 0 ? (r_ie - r_ig r_eg) / sqrt(q) : 0;     else r = r_ie.
 *                      NaN, inf, a constant series and T = 1 give 0, never NaN.  Only offsets' monotony is checked (no boxes).
 *   footprint_select:  above_i = corr_i >= thr (0 < thr <= 1); the footprint of box n is the set of above voxels connected through
 *                      faces, inside the box, to an above voxel of cores[n] (HOST [N][6], inside its box).  w[V] = corr on the
 *                      footprint, 0 elsewhere; size[n] (int32) its voxel count; wsum[n] (double) the sum of box n's w in the box's
 *                      linear order from 0.0.  One workgroup per neuron with a byte per box voxel in the LDS, swept to the fixpoint:
 *                      a box above CWFA_FOOTPRINT_SELECT_MAX voxels is refused with CWFA_E_SHAPE. */
#define CWFA_FOOTPRINT_SELECT_MAX (1 << 15)
int cwfa_roi_mark_u8(const int32_t* boxes, int N, uint8_t* occ, int D, int H, int W, void* stream);
int cwfa_roi_weighted_sums_f32(const float* x, const int32_t* boxes, const int64_t* offsets, const float* w, double* out, int T, int D,
                               int H, int W, int N, int64_t t_stride, void* stream);
int cwfa_roi_shell_sums_f32(const float* x, const int32_t* outer, const int32_t* inner, const uint8_t* occ, double* sums, int32_t* counts,
                            int T, int D, int H, int W, int N, int64_t t_stride, void* stream);
int cwfa_footprint_update_f32(const float* x, const int32_t* boxes, const int64_t* offsets, const double* c, const double* u, float* x0,
                              double* acc, double* ref, int T, int D, int H, int W, int N, int64_t t_stride, int first, void* stream);
int cwfa_footprint_corr_f32(const double* acc, const double* ref, const int64_t* offsets, int N, int64_t T, int neuropil, float* corr,
                            void* stream);
int cwfa_footprint_select_f32(const float* corr, const int32_t* boxes, const int32_t* cores, const int64_t* offsets, int N, float thr,
                              float* w, double* wsum, int32_t* size, void* stream);

/* ---- trace post-processing: behind extract_traces, on float64 rows x [N][T] with `stride` >= T elements between
 * rows (DEVICE, 8-byte aligned, CWFA_E_ALIGN otherwise).  N >= 0, T >= 1 (CWFA_E_SHAPE otherwise); arguments are checked before any
 * device work, nothing is allocated, nothing synchronises, no atomics; N == 0: no launch, CWFA_OK.  Every float64 operation is rounded
 * separately.  The order is that of cwfa_temporal_select widened to 64 bits: the unsigned image of the float64 bits of v + 0.0 (-0
 * and +0 are one value, returned as +0); every NaN sorts last and is returned as 0x7ff8000000000000.  A result of the two selections
 * is an element of the series, bit for bit.
 *
 *   sliding_quantile:  out[n][t] (contiguous [N][T]) = the k-th smallest (from 0) of x[n][lo .. hi], lo = max(0, t - h),
 *                      hi = min(T - 1, t + h), k = (p * (hi - lo)) / 100 in integers; h >= 0, 0 <= p <= 100 (CWFA_E_INVAL otherwise).
 *                      form 0: chosen here; 1: a workgroup stages a segment of `tile` outputs and its halo in the LDS, ranks the
 *                      staged keys and bisects on 16-bit ranks, h <= max_half_lds (CWFA_E_SHAPE beyond); 2: a thread per output
 *                      counts its window from memory, any h.  sliding_quantile_limits (host only) reports tile and max_half_lds.
 *   trace_select:      out[k][n] (double [K][N]) = the ranks[k]-th smallest of row n; ranks: HOST int [K], 1 <= K <= 4, each in
 *                      0 .. T - 1 (CWFA_E_INVAL otherwise).  One workgroup per row.
 *   ar1_deconv:        per row the minimiser of 1/2 sum (y_t - c_t)^2 + lam sum s_t under s_0 = c_0 >= 0, s_t = c_t - gamma c_{t-1} >= 0,
 *                      by the pool algorithm in the operation order of DESIGN.md section 28.1.  0 <= gamma < 1 (CWFA_E_INVAL
 *                      otherwise, NaN included); lam: DEVICE double [N]; pw: DEVICE double [T + 1], pw[0] = 1, pw[k] = pw[k-1] * gamma
 *                      (the caller's table); c, s: double [N][T] contiguous; pools: int32 [N], the number of pools of the row.  A row
 *                      with a non-finite sample, or a lam that is NaN, infinite or negative, gets NaN in c and s and pools = 0.  A
 *                      thread owns a row; ws: ar1_deconv_workspace_bytes(N, T) DEVICE bytes, 8-byte aligned: the pool stacks, transposed
 *                      (20 N T bytes rounded up to a multiple of 8; the kernel writes nothing behind them). */
int cwfa_sliding_quantile_limits(int* tile, int* max_half_lds);
int cwfa_sliding_quantile_f64(const double* x, int N, int T, int64_t stride, int h, int p, double* out, int form, void* stream);
int cwfa_trace_select_f64(const double* x, int N, int T, int64_t stride, const int* ranks, int K, double* out, void* stream);
int64_t cwfa_ar1_deconv_workspace_bytes(int N, int T);
int cwfa_ar1_deconv_f64(const double* y, int N, int T, int64_t stride, double gamma, const double* lam, const double* pw, double* c,
                        double* s, int32_t* pools, void* ws, void* stream);

/* ---- demixing of overlapping footprints: between the footprints and the traces' post-processing.  With w_n a
 * footprint's weights (the ragged fp32 array of cwfa_footprint_select_f32), wsum_n their sum and F the traces sum w x / wsum, the
 * voxels are modelled as sum_m w_m(v) c_m(t), so that F_n = f_n + sum_{m != n} M_nm f_m.  Every float64 operation is rounded
 * separately; no atomics; two runs are bitwise equal.
 *
 *   footprint_overlaps: G[p] (DEVICE double [P]) = sum over the intersection of boxes n and m of w_n(v) w_m(v) for pairs[p] = (n, m),
 *                      each product exact in float64, added by one wave in a fixed tree; an empty intersection gives 0.0.  boxes,
 *                      offsets: the HOST tables of the footprints (boxes well-formed and below 2^31 voxels each, offsets their
 *                      running volume); pairs: HOST int32 [P][2], 0 <= n <= m < N, strictly ascending in (n, m), P < 2^31.  ws: DEVICE,
 *                      P * CWFA_DEMIX_PAIR_BYTES bytes, 8-byte aligned: the entry point writes one record per pair (the intersection
 *                      and where it starts in either box) from the checked tables and copies them there on the stream, waiting
 *                      for the copy; the kernel indexes with nothing else.
 *   demix_plan_create: checks the directed CSR structure of the coupled neurons (HOST rowptr int32 [N+1] from 0 and monotone, col
 *                      int32 [rowptr[N]] in 0 .. N-1, ascending within a row, never the row itself) against the pair table (every
 *                      entry (n, m) has its pair (min, max) and the diagonal pair (m, m)), and keeps a DEVICE copy of its own:
 *                      the only index arrays the two kernels below read.  Allocates and synchronises: once per recording.
 *                      demix_plan_destroy frees it; a pointer that is not a live plan is refused by every entry point.
 *   demix_coeffs:      the CSR values, a thread per entry: M_nm = (G_nm wsum_m) / (G_mm wsum_n) for the entry (n, m), 0.0 where
 *                      G_nm == 0, where G_mm, wsum_n or their product is not > 0 and where sizes[n] or sizes[m] is 0.  G: DEVICE
 *                      double [P] in the order of the plan's pair table; wsum double [N], sizes int32 [N]: DEVICE.  The values stay
 *                      in the plan; val_out (nullable, DEVICE double [E]) receives a copy.
 *   demix_solve:       projected Gauss-Seidel, one thread per time step.  F: DEVICE double [N][T], f_stride >= T elements between rows;
 *                      out: double [N][T] contiguous, not F; sweeps: int32 [T].  out = F (NaN in the rows with sizes == 0), then per
 *                      sweep and n = 0 .. N-1: acc = 0.0; over the row's entries by ascending m, acc = acc + M_nm out_m where M_nm
 *                      != 0.0 (selected: a NaN behind a zero coefficient reaches nobody); new = F_n - acc, with nonneg new < 0
 *                      becomes 0.0 (NaN stays; every NaN is stored as 0x7ff8000000000000); out_n = new.  A time step ends after the
 *                      first sweep in which every |new - old| <= tol (a NaN difference is not; the rows with sizes == 0 do not
 *                      count) or after n_sweeps >= 1; sweeps[t] is the number it ran.  tol >= 0. */
#define CWFA_DEMIX_PAIR_BYTES 48
typedef struct cwfa_demix_plan cwfa_demix_plan;
int cwfa_footprint_overlaps_f32(const float* w, const int32_t* boxes, const int64_t* offsets, int N, const int32_t* pairs, int64_t P,
                                void* ws, double* G, void* stream);
int cwfa_demix_plan_create(const int32_t* rowptr, const int32_t* col, int N, const int32_t* pairs, int64_t P, cwfa_demix_plan** plan);
int cwfa_demix_plan_destroy(cwfa_demix_plan* plan);
int cwfa_demix_coeffs_f64(cwfa_demix_plan* plan, const double* G, int64_t P, const double* wsum, const int32_t* sizes, int N,
                          double* val_out, void* stream);
int cwfa_demix_solve_f64(const double* F, int64_t f_stride, double* out, int N, int T, const cwfa_demix_plan* plan, int n_sweeps,
                         double tol, int nonneg, int32_t* sweeps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CWFA_HIP_H */
