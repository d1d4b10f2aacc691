"""Tensor-level wrappers over the C ABI (include/cwfa_hip.h).  PyTorch-ROCm provides device memory and the current
HIP stream; every computation happens in libcwfa_hip.so.  Inputs must be fp32 tensors on a HIP device -- a CPU tensor
raises (there is no CPU path in the product; the CPU restatement lives in oracle/ and is test infrastructure)."""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib
from ._lib import AffineStage, Chain, ConvOpts, check

__all__ = ["haar1d", "haar2d", "gather", "affine", "channel_affine", "chain_inv", "chain_inv_var", "chain_inv_roi_cov", "chain_inv_samples", "rand_uniform", "rand_trunc_normal", "rand_poisson", "chain_nll_map", "nll_compose", "chain_fwd", "pack_conv_weight",
           "conv2d", "conv2d_wgrad", "elu_bwd", "set_precision", "gelu_add", "gelu_bwd", "layernorm_bwd", "attention_bwd", "plane_affine", "bn_bwd_stats", "bn_act_bwd", "maxpool2_bwd", "chain_bwd", "chain_inv_bwd", "prelu_bwd", "conv3d_1k1_backward", "pack_1x1_panel", "pack_split_layer_weight", "subnet_layer", "conv3d_1k1", "channel_stats", "bn_fold", "bn_running_update", "maxpool", "sample_stats", "layernorm_apply",
           "convnext_tail", "conv_writes_sample_stats", "attention_combine", "scale_channels", "axpby", "stage", "lion_step", "global_extrema", "wmse_loss"]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(t, name="tensor"):
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: cwfa_amd runs on MI355X only -- got a {t.device} tensor (no CPU fallback exists)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    return t


def planes(t, name="tensor"):
    """Return (tensor, batch_stride) with contiguous [H,W] planes and channel stride H*W (channel-sliced views of a
    contiguous NCHW tensor qualify without a copy)."""
    _dev(t, name)
    if t.dim() != 4:
        raise ValueError(f"{name}: expected [B,C,H,W], got {tuple(t.shape)}")
    B, Cc, H, W = t.shape
    ok = (W == 1 or t.stride(3) == 1) and (H == 1 or t.stride(2) == W) and (Cc == 1 or t.stride(1) == H * W)
    if not ok or (B > 1 and t.stride(0) < Cc * H * W):
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else Cc * H * W)


def _idx(perm, name="perm"):
    if perm is None:
        return None
    if not perm.is_cuda or perm.dtype != torch.int64:
        raise RuntimeError(f"{name}: index table must be an int64 tensor on the HIP device")
    return perm if perm.is_contiguous() else perm.contiguous()


# ------------------------------------------------------------------------------------------------ wavelets
def haar1d(x, rev=False, lo=None, hi=None):
    """fwd: x[B,D,H,W] -> one [B,D,H,W] tensor (lo | hi halves).  rev: that layout (or separate lo, hi) -> x."""
    L = _lib.lib()
    if not rev:
        x, xbs = planes(x, "x")
        B, D, H, W = x.shape
        out = torch.empty((B, D, H, W), dtype=x.dtype, device=x.device)
        h = D // 2
        check(L.cwfa_haar1d_fwd_f32(_p(x), _p(out), C.c_void_p(out.data_ptr() + 4 * h * H * W), B, D, H * W, xbs,
                                    D * H * W, D * H * W, _stream()), "haar1d_fwd")
        return out
    if lo is None:
        x, xbs = planes(x, "x")
        B, D, H, W = x.shape
        h = D // 2
        lo_p, hi_p, lbs, hbs = _p(x), C.c_void_p(x.data_ptr() + 4 * h * H * W), xbs, xbs
        keep = (x,)
    else:
        lo, lbs = planes(lo, "lo")
        hi, hbs = planes(hi, "hi")
        B, h, H, W = lo.shape
        D = 2 * h
        lo_p, hi_p = _p(lo), _p(hi)
        keep = (lo, hi)
    out = torch.empty((B, D, H, W), dtype=torch.float32, device=keep[0].device)
    check(L.cwfa_haar1d_inv_f32(lo_p, hi_p, _p(out), B, D, H * W, lbs, hbs, D * H * W, _stream()), "haar1d_inv")
    return out


def haar2d(x, rev, order_by_wavelet, fac):
    L = _lib.lib()
    x = _dev(x, "x").contiguous()
    if not rev:
        B, Cc, H, W = x.shape
        out = torch.empty((B, 4 * Cc, H // 2, W // 2), dtype=x.dtype, device=x.device)
        check(L.cwfa_haar2d_fwd_f32(_p(x), _p(out), B, Cc, H, W, int(order_by_wavelet), float(fac), _stream()),
              "haar2d_fwd")
        return out
    B, C4, h, w = x.shape
    out = torch.empty((B, C4 // 4, 2 * h, 2 * w), dtype=x.dtype, device=x.device)
    check(L.cwfa_haar2d_inv_f32(_p(x), _p(out), B, C4 // 4, 2 * h, 2 * w, int(order_by_wavelet), float(fac), _stream()),
          "haar2d_inv")
    return out


def haar3d(x, rev=False, order_by_wavelet=True, fac=0.5):
    """The 2 x 2 x 2 Haar tile in one launch: fwd x[B,D,H,W] -> haar2d(haar1d(x)) [B,4D,H/2,W/2]; rev the inverse.
    Bit-identical to the two-launch composition (``fac`` = haar2d's factor: 0.5 * rebalance)."""
    L = _lib.lib()
    if not rev:
        x, xbs = planes(x, "x")
        B, D, H, W = x.shape
        out = torch.empty((B, 4 * D, H // 2, W // 2), dtype=torch.float32, device=x.device)
        check(L.cwfa_haar3d_fwd_f32(_p(x), _p(out), B, D, H, W, int(order_by_wavelet), float(fac), xbs, _stream()), "haar3d_fwd")
        return out
    y = _dev(x, "y").contiguous()
    B, D4, h, w = y.shape
    if D4 % 8:
        raise ValueError(f"haar3d: {D4} channels are not 4 x an even depth")
    out = torch.empty((B, D4 // 4, 2 * h, 2 * w), dtype=torch.float32, device=y.device)
    check(L.cwfa_haar3d_inv_f32(_p(y), _p(out), B, D4 // 4, 2 * h, 2 * w, int(order_by_wavelet), float(fac), out.stride(0), _stream()),
          "haar3d_inv")
    return out


def gather(x, perm, axis):
    L = _lib.lib()
    x, xbs = planes(x, "x")
    perm = _idx(perm)
    B, Cc, H, W = x.shape
    if perm.numel() != x.shape[axis]:
        raise ValueError(f"perm of length {perm.numel()} does not match axis {axis} of {tuple(x.shape)}")
    out = torch.empty((B, Cc, H, W), dtype=x.dtype, device=x.device)
    check(L.cwfa_gather_f32(_p(x), _p(perm), _p(out), B, Cc, H, W, axis, xbs, Cc * H * W, _stream()), "gather")
    return out


# ------------------------------------------------------------------------------------------------ affine / chains
def stage(s_raw=None, t=None, clamp_kind="ATAN", clamp=2.0, pre_scale=1.0, t_neg_div_sqrt2=False, perm=None, axis=1,
          gin=False):
    """Describe one coupling stage (see cwfa_affine_stage).  Returns (ctypes struct, keep-alive tuple)."""
    st = AffineStage()
    keep = []
    if s_raw is not None:
        s_raw, sbs = planes(s_raw, "s_raw")
        st.s_raw, st.s_bs = s_raw.data_ptr(), sbs
        keep.append(s_raw)
    if t is not None:
        t, tbs = planes(t, "t")
        st.t, st.t_bs = t.data_ptr(), tbs
        keep.append(t)
    st.clamp_kind = _lib.CLAMP[clamp_kind]
    st.clamp = float(clamp)
    st.pre_scale = float(pre_scale)
    st.t_neg_div_sqrt2 = int(bool(t_neg_div_sqrt2))
    if perm is not None:
        perm = _idx(perm)
        st.perm = perm.data_ptr()
        keep.append(perm)
    st.perm_axis = int(axis)
    st.gin = int(bool(gin))
    return st, tuple(keep)


def affine(x, st_keep, rev, shape=None, logdet=None, sumsq=None, out=None):
    """y = A(gather(x)) for one stage.  x may be None (zeros) if `shape` is given.  `out` may be a channel-slice view
    (also x itself when the stage has no gather)."""
    L = _lib.lib()
    st, keep = st_keep
    if x is not None:
        x, xbs = planes(x, "x")
        shape = tuple(x.shape)
        dev = x.device
    else:
        xbs = 0
        dev = keep[0].device
    B, Cc, H, W = shape
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        ybs = Cc * H * W
    else:
        o2, ybs = planes(out, "out")
        if o2.data_ptr() != out.data_ptr() or tuple(out.shape) != tuple(shape):
            raise ValueError("affine: `out` must be a [B,C,H,W] view with contiguous planes")
    check(L.cwfa_affine_f32(_p(x), _p(out), C.byref(st), int(bool(rev)), B, Cc, H, W, xbs, ybs, _p(logdet),
                            _p(sumsq), _stream()), "affine")
    return out


def affine_bwd(x, g, st_keep, rev, gld=None, want=(True, True, True)):
    """Backward of ``affine(x, st, rev)`` for a stage without a gather: (dL/dx, dL/d s_raw, dL/d t) from g = dL/dy and the
    upstream gradient ``gld`` [B] of the per-sample log-det; entries of ``want`` switch the three outputs."""
    L = _lib.lib()
    st, keep = st_keep
    x, xbs = planes(x, "x")
    g, gbs = planes(g, "g")
    B, Cc, H, W = x.shape
    if tuple(g.shape) != (B, Cc, H, W):
        raise ValueError("affine_bwd: g and x differ in shape")
    mk = lambda on: torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device) if on else None    # noqa: E731
    gx, gs, gt = mk(want[0]), mk(want[1] and bool(st.s_raw)), mk(want[2] and bool(st.t))
    if gld is not None:
        gld = _dev(gld, "gld").contiguous()
    check(L.cwfa_affine_bwd_f32(_p(x), _p(g), C.byref(st), int(bool(rev)), B, Cc, H, W, xbs, gbs, _p(gld), _p(gx), _p(gs), _p(gt),
                                _stream()), "affine_bwd")
    return gx, gs, gt


def channel_affine(x, scale, shift, inverse=False, perm_in=None, perm_out=None):
    L = _lib.lib()
    x, xbs = planes(x, "x")
    B, Cc, H, W = x.shape
    for t in (scale, shift, perm_in, perm_out):
        if t is not None and t.numel() != Cc:
            raise ValueError("channel_affine: scale / shift / permutation tables must hold one entry per channel")
    out = torch.empty((B, Cc, H, W), dtype=x.dtype, device=x.device)
    check(L.cwfa_channel_affine_f32(_p(x), _p(out), _p(scale), _p(shift), int(bool(inverse)), _p(_idx(perm_in)),
                                    _p(_idx(perm_out)), B, Cc, H * W, xbs, Cc * H * W, _stream()), "channel_affine")
    return out


def _chain(stages, tables=None):
    if len(stages) > _lib.CHAIN_MAX:
        raise ValueError(f"chain of {len(stages)} stages exceeds CWFA_CHAIN_MAX={_lib.CHAIN_MAX}")
    ch = Chain()
    ch.n_stages = len(stages)
    keep = []
    for k, (st, kp) in enumerate(stages):
        ch.stage[k] = st
        keep.append(kp)
    if tables is not None:
        ch.src_c, ch.src_h = (t.data_ptr() for t in tables)
        keep.append(tables)
    return ch, keep


def chain_tables(perms, final_perm, C_, H, W, device):
    """The gathers of a chain composed per axis (see cwfa_chain.src_* in include/cwfa_hip.h).  ``perms``: per stage in
    execution order (table or None, axis).  Returns two int32 device tensors [n+1, C], [n+1, H]; built once per plan and
    direction (a handful of tiny index ops) and reused by every launch.  (Column permutations are not composed: the
    kernels move the values between threads instead.)"""
    idx = {1: torch.arange(C_, device=device), 2: torch.arange(H, device=device)}
    if final_perm is not None:
        idx[1] = final_perm.to(device)[idx[1]]
    n = len(perms)
    rows = {1: [None] * (n + 1), 2: [None] * (n + 1)}
    for k in range(n - 1, -1, -1):
        for ax in (1, 2):
            rows[ax][k] = idx[ax]
        table, axis = perms[k]
        if table is not None and axis in (1, 2):
            idx[axis] = table.to(device)[idx[axis]]
    for ax in (1, 2):
        rows[ax][n] = idx[ax]
    return tuple(torch.stack(rows[ax]).to(torch.int32).contiguous() for ax in (1, 2))


def chain_inv(z, low, stages, logdet=None, tables=None):
    """x[B,2C,H,W] = Haar1D^-1(cat[low, A_{K-1}^-1(...A_0^-1(z))]); z may be None (= zeros).  ``tables``: chain_tables()
    of the stages' gathers (optional, speed only)."""
    L = _lib.lib()
    low, lbs = planes(low, "low")
    B, Cc, H, W = low.shape
    zbs = 0
    if z is not None:
        z, zbs = planes(z, "z")
        if tuple(z.shape) != tuple(low.shape):
            raise ValueError(f"z {tuple(z.shape)} and low {tuple(low.shape)} differ")
    ch, keep = _chain(stages, tables)
    out = torch.empty((B, 2 * Cc, H, W), dtype=torch.float32, device=low.device)
    rec = chain_event_sink
    if rec is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(L.cwfa_chain_inv_f32(_p(z), _p(low), _p(out), C.byref(ch), B, Cc, H, W, zbs, lbs, 2 * Cc * H * W, _p(logdet),
                               _stream()), "chain_inv")
    if rec is not None:
        e1.record()
        rec.append(("inv", B, Cc, H, W, len(stages), z is not None, e0, e1))
    return out


def chain_inv_var(var_low, stages, z_var, shape=None, std_scale=0.0, tables=None):
    """Per-voxel variance [B,2C,H,W] of ``chain_inv(z, low, stages)`` for independent latents of variance ``z_var`` and an
    independent per-voxel variance ``var_low`` [B,C,H,W] of ``low`` (None = 0: then ``shape = (B, C, H, W)`` is needed and the
    device is that of the stages' tensors).  The shifts of the stages are never read.  ``std_scale`` > 0 returns
    ``std_scale * sqrt(variance)`` instead (see cwfa_chain_inv_var_f32).  ``tables`` as for ``chain_inv``."""
    L = _lib.lib()
    if var_low is not None:
        var_low, vbs = planes(var_low, "var_low")
        if shape is not None and tuple(shape) != tuple(var_low.shape):
            raise ValueError(f"var_low {tuple(var_low.shape)} and shape {tuple(shape)} differ")
        shape, dev = tuple(var_low.shape), var_low.device
    else:
        if shape is None or len(shape) != 4:
            raise ValueError("chain_inv_var: without var_low the shape (B, C, H, W) must be given")
        vbs = 0
        dev = next((t.device for _, kp in stages for t in kp), None) if tables is None else tables[0].device
        if dev is None:                     # a chain without a single tensor: the current device
            dev = torch.device("cuda", torch.cuda.current_device())
    B, Cc, H, W = (int(v) for v in shape)
    ch, keep = _chain(stages, tables)
    out = torch.empty((B, 2 * Cc, H, W), dtype=torch.float32, device=dev)
    check(L.cwfa_chain_inv_var_f32(_p(var_low), _p(out), C.byref(ch), float(z_var), float(std_scale), B, Cc, H, W, vbs,
                                   2 * Cc * H * W, _stream()), "chain_inv_var")
    return out


ROI_COV_ARG_PAIRS = 64        # ROI_COV_CHUNK of csrc/elementwise.hip: up to this many pairs travel in one launch's kernel arguments


class RoiPairs:
    """The box / pair tables of ``chain_inv_roi_cov`` prepared once for the steps of a pyramid: the int32 host tables the library
    validates and, with ``device_table``, the device copy [P, 12] of the pairs' boxes (one upload for every step)."""

    def __init__(self, boxes, pairs=None, device=None, device_table=None):
        import numpy as np
        self.boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 6))
        self.pairs = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        self.n_pairs = len(self.boxes) if self.pairs is None else len(self.pairs)
        if device_table is None:                 # beyond one launch's worth of kernel arguments
            device_table = self.n_pairs > ROI_COV_ARG_PAIRS
        self.table = None
        if device_table and self.n_pairs:
            R = len(self.boxes)
            idx = np.repeat(np.arange(R)[:, None], 2, 1) if self.pairs is None else self.pairs
            if idx.size and (idx.min() < 0 or idx.max() >= R):
                raise ValueError(f"chain_inv_roi_cov: a pair names a box outside [0, {R})")
            tab = np.ascontiguousarray(self.boxes[idx].reshape(-1, 12))
            self.table = torch.from_numpy(tab).to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))


def chain_inv_roi_cov(out, stages, z_var, shape, level, boxes, pairs=None, tables=None):
    """Accumulate into ``out`` (float64 [B, P] on the device, zeroed by the caller; returned) one step's term of the covariance of
    the ROI means of the final volume (cwfa_chain_inv_roi_cov_f32).  ``stages``: the step's inverse chain with coefficients of
    ``shape = (B, C, H, W)``; ``level`` = m: 1 for the finest step, so that the final volume has C * 2^m depths; ``boxes``: the
    integer [R, 6] host table of ``roi_means`` in the final volume's coordinates, ``pairs``: integer [P, 2] box indices (None = the
    R diagonal pairs: the variances) -- or a prepared ``RoiPairs`` as ``boxes``.  A pair with an empty box becomes NaN.  ``tables``
    is accepted for symmetry with the other chain ops; the kernel walks the gathers itself."""
    L = _lib.lib()
    if not torch.is_tensor(out) or not out.is_cuda:
        raise RuntimeError("chain_inv_roi_cov: cwfa_amd runs on MI355X only -- `out` must be a device tensor (no CPU fallback exists)")
    if out.dtype != torch.float64 or out.dim() != 2 or not out.is_contiguous():
        raise TypeError("chain_inv_roi_cov: `out` must be a contiguous float64 [B, P] tensor")
    rp = boxes if isinstance(boxes, RoiPairs) else RoiPairs(boxes, pairs, out.device)
    if isinstance(boxes, RoiPairs) and pairs is not None:
        raise ValueError("chain_inv_roi_cov: a prepared RoiPairs already holds its pairs")
    B, Cc, H, W = (int(v) for v in shape)
    if tuple(out.shape) != (B, rp.n_pairs):
        raise ValueError(f"chain_inv_roi_cov: out {tuple(out.shape)} is not [B, P] = {(B, rp.n_pairs)}")
    ch, keep = _chain(stages, None)
    check(L.cwfa_chain_inv_roi_cov_f32(_p(out), C.byref(ch), float(z_var), B, Cc, H, W, int(level), C.c_void_p(rp.boxes.ctypes.data),
                                       len(rp.boxes), None if rp.pairs is None else C.c_void_p(rp.pairs.ctypes.data), rp.n_pairs,
                                       _p(rp.table), rp.n_pairs, _stream()), "chain_inv_roi_cov")
    return out


def _rand_args(seed, stream, sample_offset, name):
    seed, stream, sample_offset = int(seed), int(stream), int(sample_offset)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{name}: seed {seed} is not an unsigned 64-bit number")
    if not 0 <= stream < 1 << 32 or not 0 <= sample_offset < 1 << 32:
        raise ValueError(f"{name}: stream {stream} / sample_offset {sample_offset} are not unsigned 32-bit numbers")
    return C.c_uint64(seed), C.c_uint32(stream), C.c_uint32(sample_offset)


def _rand_out(shape, device, name):
    shape = tuple(int(v) for v in shape)
    if len(shape) < 1 or any(v < 0 for v in shape):
        raise ValueError(f"{name}: shape {shape} needs a leading sample axis and no negative size")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _dev(out, name)
    n = 1
    for v in shape[1:]:
        n *= v
    return out, shape[0], n


def rand_uniform(shape, seed, stream=0, sample_offset=0, device=None):
    """Uniforms in (0, 1) of the counter-based generator (cwfa_rand_uniform_f32): ``shape[0]`` is the SAMPLE axis, the rest is one
    sample.  Sample n of a call equals sample 0 of a call with ``sample_offset + n``; ``stream`` separates independent uses of
    one seed."""
    out, N, n = _rand_out(shape, device, "rand_uniform")
    if out.numel() == 0:
        return out
    check(_lib.lib().cwfa_rand_uniform_f32(_p(out), N, n, n, *_rand_args(seed, stream, sample_offset, "rand_uniform"), _stream()),
          "rand_uniform")
    return out


def rand_trunc_normal(shape, temperature, seed, stream=0, sample_offset=0, device=None):
    """Standard normals truncated to [-temperature, temperature] (the draw of ``CWFA.sample_z_truncated``) from the same generator
    and counters as ``rand_uniform``, in one launch.  ``temperature`` > 0 (inf allowed)."""
    out, N, n = _rand_out(shape, device, "rand_trunc_normal")
    seed, stream, sample_offset = _rand_args(seed, stream, sample_offset, "rand_trunc_normal")
    if out.numel() == 0 and float(temperature) > 0.0:
        return out
    check(_lib.lib().cwfa_rand_trunc_normal_f32(_p(out), N, n, n, float(temperature), seed, stream, sample_offset, _stream()),
          "rand_trunc_normal")
    return out


def _poisson_tensor(t, name):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"rand_poisson: {name} must be a contiguous float32 tensor on the HIP device (no CPU path exists), got "
                         f"{(t.dtype, t.device, 'contiguous' if t.is_contiguous() else 'strided') if torch.is_tensor(t) else type(t)}")
    return t


def _sample_scale(v, N, device, name):
    """``pre`` / ``post`` of rand_poisson as a float32 device tensor [N] (a Python number is filled in on the device: no read-back)."""
    if v is None:
        return None
    if not torch.is_tensor(v):
        return torch.full((N,), float(v), dtype=torch.float32, device=device)
    if _poisson_tensor(v, name).dim() != 1 or v.shape[0] != N or v.device != device:
        raise ValueError(f"rand_poisson: {name} must be a float32 tensor [{N}] on {device}, got {tuple(v.shape)} on {v.device}")
    return v


def rand_poisson(lam, seed, stream=0, sample_offset=0, n_samples=None, pre=None, post=None, out=None):
    """Poisson draws of the counter-based generator (cwfa_rand_poisson_f32):
    ``out[s] = fl32(fl32(k) * post[s])``, ``k ~ Poisson(fl32(lam[s] * pre[s]))``.  ``lam``: contiguous float32 on the HIP device, its
    leading axis the SAMPLE axis; with ``n_samples`` it is ONE plane shared by all samples and the result is [n_samples, *lam.shape].
    ``pre`` / ``post``: float32 device tensors [N] or Python numbers (None: 1).  ``out``: a contiguous float32 tensor of the result's
    shape; ``out=lam`` draws in place (not with ``n_samples``).  Sample s of a call equals sample 0 of a call with
    ``sample_offset + s``; ``stream`` separates independent uses of one seed.  The counters are NOT those of ``rand_uniform``.
    Rate 0 gives 0; a rate that is negative, NaN or above 2^30 gives NaN (nothing is read back to validate); rates below 10 are drawn
    by inversion of a 32-bit uniform, so outcomes of probability below 2^-33 are unreachable; ``fl32(k)`` is exact only below 2^24."""
    _poisson_tensor(lam, "lam")
    if n_samples is None:
        if lam.dim() < 1:
            raise ValueError("rand_poisson: lam needs a leading sample axis (or pass n_samples)")
        N, shape = int(lam.shape[0]), tuple(lam.shape)
        n = lam.numel() // N if N else 0
        lam_ss = n
    else:
        N = int(n_samples)
        if N < 0:
            raise ValueError(f"rand_poisson: n_samples = {n_samples}")
        shape, n, lam_ss = (N,) + tuple(lam.shape), lam.numel(), 0
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=lam.device)
    else:
        if tuple(_poisson_tensor(out, "out").shape) != shape or out.device != lam.device:
            raise ValueError(f"rand_poisson: out must be a float32 tensor {shape} on {lam.device}")
    pre, post = _sample_scale(pre, N, lam.device, "pre"), _sample_scale(post, N, lam.device, "post")
    args = _rand_args(seed, stream, sample_offset, "rand_poisson")
    if out.numel() == 0:
        return out
    check(_lib.lib().cwfa_rand_poisson_f32(_p(out), _p(lam), N, n, lam_ss, n, _p(pre), _p(post), *args, _stream()), "rand_poisson")
    return out


def chain_inv_samples(low, stages, n_samples, temperature, seed, stream=0, sample_offset=0, tables=None, return_z=False):
    """``n_samples`` draws [N,B,2C,H,W] of ``chain_inv(z, low, stages)`` in ONE launch, z drawn in the kernel as by
    ``rand_trunc_normal((N,B,C,H,W), temperature, seed, stream, sample_offset)`` and indexed by the position at which a latent
    ARRIVES at the end of the chain.  ``low``: [B,C,H,W] (shared by all samples) or [N,B,C,H,W] (each sample its own).  With
    ``return_z`` also z [N,B,C,H,W] laid out where the latents START, so that ``chain_inv(z[n], low[n], stages)`` reproduces sample
    n.  ``temperature`` must be > 0: at 0 every sample is ``chain_inv(None, low, stages)``.  ``tables`` as for ``chain_inv``."""
    L = _lib.lib()
    N = int(n_samples)
    if N < 1:
        raise ValueError("chain_inv_samples: n_samples must be >= 1")
    if not float(temperature) > 0.0:
        raise ValueError(f"chain_inv_samples: temperature {temperature!r} must be > 0 (use chain_inv(None, ...) for the mean)")
    _dev(low, "low")
    if low.dim() == 5:
        if low.shape[0] != N:
            raise ValueError(f"chain_inv_samples: low holds {low.shape[0]} samples, n_samples = {N}")
        low = low.contiguous()
        _, B, Cc, H, W = low.shape
        lss, lbs = B * Cc * H * W, Cc * H * W
    else:
        low, lbs = planes(low, "low")
        B, Cc, H, W = low.shape
        lss = 0
    ch, keep = _chain(stages, tables)
    out = torch.empty((N, B, 2 * Cc, H, W), dtype=torch.float32, device=low.device)
    z = torch.empty((N, B, Cc, H, W), dtype=torch.float32, device=low.device) if return_z else None
    n = Cc * H * W
    seed, stream, sample_offset = _rand_args(seed, stream, sample_offset, "chain_inv_samples")
    check(L.cwfa_chain_inv_samples_f32(_p(low), _p(out), _p(z), C.byref(ch), N, B, Cc, H, W, lss, lbs, 2 * B * n, 2 * n, B * n, n,
                                       float(temperature), seed, stream, sample_offset, _stream()), "chain_inv_samples")
    return (out, z) if return_z else out


def chain_nll_map(x, stages, tables=None, want_low=True, want_z=False, want_nll=True, nll_sum=None):
    """(nll, low, z) of the volume ``x`` [B,2C,H,W] under one CAT step (cwfa_chain_nll_map_f32), each
    [B,C,H,W] or None where not wanted.  ``stages`` are the INVERSE-direction stages (``_CatStepPlan.inverse_stages``), ``tables``
    as for ``chain_inv``.  With d = (x[2c] - x[2c+1]) / sqrt 2 and the step's posterior d = g z + o:  z = (d - o) / g is the
    standardised residual of the coefficient AT ITS OWN POSITION, nll = z^2 / 2 + log g its share of the step's negative
    log-likelihood (no log 2 pi term) and low = (x[2c] + x[2c+1]) / sqrt 2 the next step's input, bit-equal to ``chain_fwd``'s.
    ``nll_sum``: float64 [B] on the device, onto which the per-sample sums of nll are ACCUMULATED.  One launch."""
    L = _lib.lib()
    x, xbs = planes(x, "x")
    B, D, H, W = x.shape
    if D % 2:
        raise ValueError(f"chain_nll_map: x has {D} channels, an odd number")
    Cc = D // 2
    if nll_sum is not None:
        if not torch.is_tensor(nll_sum) or not nll_sum.is_cuda or nll_sum.dtype != torch.float64:
            raise TypeError("chain_nll_map: nll_sum must be a float64 tensor on the HIP device")
        if tuple(nll_sum.shape) != (B,) or not nll_sum.is_contiguous() or nll_sum.device != x.device:
            raise ValueError(f"chain_nll_map: nll_sum must be a contiguous [{B}] tensor on x's device, got {tuple(nll_sum.shape)}")
    ch, keep = _chain(stages, tables)
    mk = lambda on: torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device) if on else None    # noqa: E731
    nll, low, z = mk(want_nll), mk(want_low), mk(want_z)
    n = Cc * H * W
    check(L.cwfa_chain_nll_map_f32(_p(x), _p(low), _p(z), _p(nll), C.byref(ch), B, Cc, H, W, xbs, n, n, n, _p(nll_sum), _stream()),
          "chain_nll_map")
    return nll, low, z


def nll_compose(levels):
    """The per-step maps of a pyramid (finest first; level n is [B, D >> (n+1), H, W]) as one volume [B,D,H,W]:
    out[b,d] = sum_n 2^-(n+1) level_n[b, d >> (n+1)], added finest first in fp32 (cwfa_nll_compose_f32), so that a sample's total
    is the total of its levels.  One launch."""
    L = _lib.lib()
    levels = list(levels)
    if not 1 <= len(levels) <= _lib.NLL_MAX_LEVELS:
        raise ValueError(f"nll_compose: {len(levels)} levels (1 .. {_lib.NLL_MAX_LEVELS})")
    tab = _lib.NllLevels()
    tab.n = len(levels)
    keep = []
    for k, lv in enumerate(levels):
        lv, bs = planes(lv, f"levels[{k}]")
        if k == 0:
            B, C0, H, W = lv.shape
            D = 2 * C0
            if D % (1 << len(levels)):
                raise ValueError(f"nll_compose: {D} depths are not divisible by 2^{len(levels)}")
        if tuple(lv.shape) != (B, D >> (k + 1), H, W) or lv.device != levels[0].device:
            raise ValueError(f"nll_compose: levels[{k}] is {tuple(lv.shape)} on {lv.device}, expected {(B, D >> (k + 1), H, W)} on "
                             f"{levels[0].device}")
        tab.level[k], tab.bs[k] = lv.data_ptr(), bs
        keep.append(lv)
    out = torch.empty((B, D, H, W), dtype=torch.float32, device=keep[0].device)
    check(L.cwfa_nll_compose_f32(C.byref(tab), _p(out), B, D, H * W, D * H * W, _stream()), "nll_compose")
    return out


def chain_fwd(x, stages, final_perm=None, logdet=None, sumsq=None, tables=None):
    """(z, low) for x[B,2C,H,W].  ``tables``: chain_tables() of the stages' gathers INCLUDING final_perm (optional)."""
    L = _lib.lib()
    x, xbs = planes(x, "x")
    B, D, H, W = x.shape
    Cc = D // 2
    ch, keep = _chain(stages, tables)
    low = torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device)
    z = torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device)
    rec = chain_event_sink
    if rec is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(L.cwfa_chain_fwd_f32(_p(x), _p(low), _p(z), C.byref(ch), _p(_idx(final_perm)), B, Cc, H, W, xbs, Cc * H * W,
                               Cc * H * W, _p(logdet), _p(sumsq), _stream()), "chain_fwd")
    if rec is not None:
        e1.record()
        rec.append(("fwd", B, Cc, H, W, len(stages), True, e0, e1))
    return z, low


chain_event_sink = None     # list collecting (direction, B, C, H, W, stages, z_read, start_event, end_event); set by bench.py only


def _chain_grads(grads, shape):
    B, Cc, H, W = shape
    gr = _lib.ChainGrads()
    for k, (ds, dt) in enumerate(grads):
        for name, t in (("ds", ds), ("dt", dt)):
            if t is None:
                continue
            t2, bs = planes(t, name)
            if t2.data_ptr() != t.data_ptr() or tuple(t.shape) != (B, Cc, H, W):
                raise ValueError(f"chain backward: {name}[{k}] must be a [B,C,H,W] view with contiguous planes")
            getattr(gr, name)[k] = t.data_ptr()
            getattr(gr, name + "_bs")[k] = bs
    return gr


def chain_inv_bwd(xhat, gt, stages, grads, gscale, loss_kind=2, accumulate=False, want_latent_grad=False, want_low_grad=False):
    """Backward of gscale-weighted sum |xhat - gt|^p (p = loss_kind) through the inverse pass that produced ``xhat``;
    ``stages`` in FORWARD order.  ``loss_kind`` 0: ``gt`` IS an upstream gradient dL/dxhat (times gscale).  Returns the float64[1]
    tensor sum |xhat - gt|^p -- or, with ``want_latent_grad`` / ``want_low_grad``, the tuple (sum, dL/dz, dL/dlow) of the inverse
    pass's two inputs (None where not wanted; dL/dlow needs loss_kind 0)."""
    L = _lib.lib()
    xhat, xbs = planes(xhat, "xhat")
    gt, gbs = planes(gt, "gt")
    if tuple(xhat.shape) != tuple(gt.shape):
        raise ValueError("chain_inv_bwd: xhat and gt differ in shape")
    B, D, H, W = xhat.shape
    Cc = D // 2
    ch, keep = _chain(stages)
    gr = _chain_grads(grads, (B, Cc, H, W))
    loss = torch.zeros(1, dtype=torch.float64, device=xhat.device)
    if want_low_grad and loss_kind != 0:
        raise ValueError("chain_inv_bwd: dL/dlow is formed from an upstream gradient (loss_kind 0)")
    gz = torch.empty((B, Cc, H, W), dtype=torch.float32, device=xhat.device) if want_latent_grad else None
    glow = torch.empty((B, Cc, H, W), dtype=torch.float32, device=xhat.device) if want_low_grad else None
    check(L.cwfa_chain_inv_bwd_f32(_p(xhat), _p(gt), C.byref(ch), C.byref(gr), B, Cc, H, W, xbs, gbs, float(gscale), int(loss_kind),
                                   int(bool(accumulate)), _p(loss), _p(gz), _p(glow), _stream()), "chain_inv_bwd")
    if want_latent_grad or want_low_grad:
        return loss, gz, glow
    return loss


def chain_bwd(z, stages, grads, final_perm=None, gscale=0.0, ldscale=0.0, gz=None, want_input_grad=False, accumulate=False, gld=None):
    """Backward of L = gscale*0.5*sum z^2 - ldscale*sum logdet (+ <gz, z>) through the chain that produced ``z``
    (``chain_fwd`` with the same ``stages`` / ``final_perm``).  ``grads[k] = (ds_raw_k, dt_k)``: preallocated
    [B,C,H,W] views (contiguous planes) or None.  Returns dL/d(detail band) if ``want_input_grad``."""
    L = _lib.lib()
    z, zbs = planes(z, "z")
    B, Cc, H, W = z.shape
    ch, keep = _chain(stages)
    gr = _chain_grads(grads, (B, Cc, H, W))
    gzbs = 0
    if gz is not None:
        gz, gzbs = planes(gz, "gz")
    gv0 = torch.empty((B, Cc, H, W), dtype=torch.float32, device=z.device) if want_input_grad else None
    if gld is not None:                      # upstream gradient of the per-sample log-det (autograd)
        gld = _dev(gld, "gld").contiguous()
        if gld.numel() != B:
            raise ValueError("chain_bwd: gld must hold one value per sample")
    check(L.cwfa_chain_bwd_f32(_p(z), _p(gz), C.byref(ch), C.byref(gr), _p(_idx(final_perm)), _p(gv0), B, Cc, H, W, zbs, gzbs,
                               Cc * H * W, float(gscale), float(ldscale), int(bool(accumulate)), _p(gld), _stream()), "chain_bwd")
    return gv0


# ------------------------------------------------------------------------------------------------ convolutions
class PackedConv:
    """Kernel-layout image of one filter bank (built once per weight version on the device)."""
    __slots__ = ("packed", "cout", "cin", "ks", "transposed", "version", "src_ptr", "split", "epoch", "version1", "src_ptr1", "cat_c1",
                 "cat_from", "short", "walk")

    def __init__(self, packed, cout, cin, ks, transposed, version, src_ptr, split=False):
        self.packed, self.cout, self.cin, self.ks = packed, cout, cin, ks
        self.transposed, self.version, self.src_ptr = transposed, version, src_ptr
        self.split = split          # weights held as three bf16 pieces for the split-bf16 kernels (set_precision)
        self.epoch = _pack_epoch    # set_option() generation this image was built under (caches re-pack on a change)
        self.walk = None            # second image of the bank for the persistent output convolution (out_walk_bank), or None


def pack_conv_weight(w, transposed=False, direct=False):
    """w: [Cout,Cin,k,k] (k in 1,3,7), or with transposed=True a ConvTranspose2d weight [Cin,Co,2,2].  ``direct``: the fp32 MFMA
    kernels' layout whatever the precision mode (banks whose launch is bound by its output stores, not by the matrix pipe).
    A bank of the persistent output convolution (out_walk_bank) carries that kernel's image as well (``walk``): both belong to the
    one PackedConv and so go stale together."""
    pc = _pack_conv_weight(w, transposed, direct)
    if not direct and out_walk_bank(pc.cout, pc.cin, pc.ks, transposed):
        L = _lib.lib()
        wc = _dev(w, "weight").detach().contiguous()
        pc.walk = torch.empty(L.cwfa_conv3x3_out_split_packed_bytes(pc.cout), dtype=torch.uint8, device=wc.device)
        check(L.cwfa_conv3x3_out_split_pack_f32(_p(wc), _p(pc.walk), pc.cout, _stream()), "conv3x3_out_split_pack")
    return pc


def _pack_conv_weight(w, transposed, direct):
    L = _lib.lib()
    w = _dev(w, "weight").detach().contiguous()
    if transposed:
        cin, co, kh, kw = w.shape
        if (kh, kw) != (2, 2):
            raise ValueError("only 2x2 stride-2 transposed convolutions are supported")
        cout, ks = 4 * co, 1
    else:
        cout, cin, ks, kw = w.shape
        if ks != kw:
            raise ValueError("square kernels only")
    if direct:
        pass
    elif _split_bf16 and ks == 1 and cout >= 128:
        packed = torch.empty(L.cwfa_conv_split_packed_bytes(cout, cin, ks), dtype=torch.uint8, device=w.device)
        check(L.cwfa_conv_split_pack_f32(_p(w), _p(packed), cout, cin, ks, int(transposed), _stream()), "conv_split_pack")
        return PackedConv(packed, cout, cin, ks, transposed, w._version, w.data_ptr(), split=True)
    # (bf16 / fp16 mode: one product per multiply-add -- there the 32-channel tiling beats the fp32 Winograd kernel for 17 .. 32 outputs too)
    narrow_max = 32 if single_product() else SPLIT_3X3_NARROW_MAX
    if not direct and _split_bf16 >= 2 and ks == 3 and cout >= SPLIT_3X3_MIN_COUT and (cout > 32 or (cout <= narrow_max and cin >= 29)):
        packed = torch.empty(L.cwfa_conv3x3_split_packed_bytes(cout, cin), dtype=torch.uint8, device=w.device)
        check(L.cwfa_conv3x3_split_pack_f32(_p(w), _p(packed), cout, cin, _stream()), "conv3x3_split_pack")
        return PackedConv(packed, cout, cin, ks, transposed, w._version, w.data_ptr(), split=True)
    if not direct and SPLIT_7X7 and _split_bf16 >= 2 and ks == 7 and cout <= 64 and cin >= 32:   # the ConvNeXt convolution of the LRNN (64 -> 64)
        packed = torch.empty(L.cwfa_conv7x7_split_packed_bytes(cout, cin), dtype=torch.uint8, device=w.device)
        check(L.cwfa_conv7x7_split_pack_f32(_p(w), _p(packed), cout, cin, _stream()), "conv7x7_split_pack")
        return PackedConv(packed, cout, cin, ks, transposed, w._version, w.data_ptr(), split=True)
    n = L.cwfa_conv2d_packed_floats(cout, cin, ks)
    if n <= 0:
        raise ValueError(f"unsupported filter bank {tuple(w.shape)}")
    packed = torch.empty(n, dtype=torch.float32, device=w.device)
    check(L.cwfa_conv2d_pack_f32(_p(w), _p(packed), cout, cin, ks, int(transposed), _stream()), "conv2d_pack")
    return PackedConv(packed, cout, cin, ks, transposed, w._version, w.data_ptr())


def pack_conv_weight_cat(w, c1):
    """1x1 bank [Cout <= 64, c1 + c2, 1, 1] for conv2d(x, pc, cat=x2): the input cat(x, x2) is read from its two tensors.  The
    columns of the first source are padded with zeros to a multiple of 16 (one K chunk of the kernel)."""
    w = _dev(w, "weight").detach()
    cout, cin, ks, kw = w.shape
    if ks != 1 or kw != 1 or cout > 64 or not (0 < c1 < cin):
        raise ValueError(f"pack_conv_weight_cat: a 1x1 bank with <= 64 outputs and 0 < c1 < Cin is needed, got {tuple(w.shape)}, c1 = {c1}")
    start = (c1 + 15) // 16 * 16
    wz = torch.zeros((cout, start + cin - c1, 1, 1), dtype=torch.float32, device=w.device)
    wz[:, :c1] = w[:, :c1]
    wz[:, start:] = w[:, c1:]
    pc = pack_conv_weight(wz)                       # (cout <= 64: always the direct kernel's layout)
    pc.version, pc.src_ptr = w._version, w.data_ptr()
    pc.cat_c1, pc.cat_from = c1, start
    return pc


def conv_writes_stats(pc, act=None, residual=None, act2=None, out_blocked=False, in_add=False):
    """True when conv2d(..., out_stats=) is available for this bank / epilogue: the split-bf16 3x3 kernel with an NCHW output and
    a bias / PReLU epilogue takes the per-channel (sum, sum of squares) of its output from the accumulators.  ``in_add``: the
    call adds a tensor on load; with a bias-only epilogue that runs on the kernel's run-time epilogue, which has no statistics."""
    return bool(pc.split and pc.ks == 3 and act in (None, "prelu") and residual is None and act2 is None and not out_blocked
                and not (in_add and act is None))


def conv_writes_sample_stats(pc):
    """True when conv2d(..., out_sample_stats=) is available for this bank: the few-channel form of the split 7x7 kernel (at most 8
    inputs with the ones channel: the composed ConvNeXt bank) adds the per-sample (sum, sum of squares) of its output from its
    epilogue.  The 9 .. 16-input form, the 64-channel 7x7 and the fp32 kernels do not; ops.sample_stats stays for them."""
    return bool(pc.split and pc.ks == 7 and pc.cin <= 8)


def conv2d(x, pc, bias=None, act=None, prelu_alpha=None, residual=None, act2=None, in_scale=None, in_shift=None,
           in_add=None, out=None, in_blocked=False, out_blocked=False, cat=None, out_stats=None, out_sample_stats=None):
    """y = act2(act(conv(x') + bias) + residual), x' = x*in_scale[c] + in_shift[c] + in_add.  Transposed banks
    (ConvTranspose2d k2 s2) write the pixel-shuffled [B,Co,2H,2W] output.  ``out_stats`` (float64 [2*Cout], see
    conv_writes_stats): the launch adds (sum y, sum y^2) per channel -- the statistics of a BatchNorm behind the convolution.
    ``out_sample_stats`` (float64 [2*B], see conv_writes_sample_stats): the launch adds (sum y, sum y^2) per sample -- the
    statistics of a LayerNorm over (C,H,W) behind the convolution."""
    L = _lib.lib()
    x, xbs = planes(x, "x")
    B, Cin, H, W = x.shape
    o = ConvOpts()
    keep = [x]
    walk = out_walk_selected(pc, H, W, act=act, prelu_alpha=prelu_alpha, residual=residual, act2=act2, in_scale=in_scale, in_add=in_add,
                             out_blocked=out_blocked, cat=cat, out_stats=out_stats, out_sample_stats=out_sample_stats)
    if cat is not None:                     # the input is cat(x, cat) read from its two tensors (pack_conv_weight_cat)
        cat, cbs = planes(cat, "cat")
        c1 = getattr(pc, "cat_c1", None)
        if c1 is None or Cin != c1 or tuple(cat.shape) != (B, pc.cin - pc.cat_from, H, W) or in_scale is not None or in_add is not None:
            raise ValueError("conv2d: `cat` needs a bank from pack_conv_weight_cat for exactly these two inputs, and no load-side prologue")
        o.in_cat, o.in_cat_bs, o.in_cat_from, o.in_cat_c1 = cat.data_ptr(), cbs, pc.cat_from, c1
        keep.append(cat)
        Cin = pc.cin
    if Cin != pc.cin:
        raise ValueError(f"conv2d: input has {Cin} channels, filter bank expects {pc.cin}")
    up = bool(pc.transposed)
    oshape = (B, pc.cout // 4, 2 * H, 2 * W) if up else (B, pc.cout, H, W)
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device=x.device)
        ybs = oshape[1] * oshape[2] * oshape[3]
    else:
        if tuple(out.shape) != oshape:
            raise ValueError(f"conv2d: out has shape {tuple(out.shape)}, expected {oshape}")
        out_c, ybs = planes(out, "out")
        if out_c.data_ptr() != out.data_ptr():
            raise ValueError("conv2d: `out` must have contiguous planes")
    if bias is not None:
        o.bias = _dev(bias, "bias").data_ptr()
    o.act, o.act2 = _lib.ACT[act], _lib.ACT[act2]
    if prelu_alpha is not None:
        prelu_alpha = _dev(prelu_alpha, "prelu_alpha")
        o.prelu_alpha = prelu_alpha.data_ptr()
        if prelu_alpha.numel() != 1:             # one slope per output channel (1.0 = no activation there): split-bf16 3x3 kernel only
            if prelu_alpha.numel() != pc.cout or not prelu_alpha.is_contiguous() or not (pc.split and pc.ks == 3):
                raise ValueError("conv2d: per-channel PReLU slopes need [Cout] contiguous values and the split-bf16 3x3 kernel")
            o.prelu_per_channel = 1
    elif "prelu" in (act, act2):
        raise ValueError("conv2d: PReLU needs prelu_alpha")
    if residual is not None:
        residual, rbs = planes(residual, "residual")
        if tuple(residual.shape) != oshape:
            raise ValueError(f"conv2d: residual {tuple(residual.shape)} != output {oshape}")
        o.residual, o.res_bs = residual.data_ptr(), rbs
        keep.append(residual)
    if in_scale is not None:
        o.in_scale, o.in_shift = _dev(in_scale).data_ptr(), _dev(in_shift).data_ptr()
        if in_scale.numel() not in (Cin, B * Cin) or in_shift.numel() != in_scale.numel():
            raise ValueError("conv2d: in_scale / in_shift must be [Cin] or [B,Cin]")
        o.in_affine_bs = Cin if (in_scale.numel() == B * Cin and B > 1) else 0
    if in_add is not None:
        in_add, abs_ = planes(in_add, "in_add")
        if tuple(in_add.shape) != tuple(x.shape):
            raise ValueError("conv2d: in_add shape mismatch")
        o.in_add, o.in_add_bs = in_add.data_ptr(), abs_
        keep.append(in_add)
    o.upshuffle2 = int(up)
    if in_blocked:                          # x is a channel-blocked map of the fused layer kernel (subnet_layer, layout bit 1)
        if not (walk or (pc.split and pc.ks == 3)):
            raise ValueError("conv2d: channel-blocked input is read by the split-bf16 3x3 kernels only")
        o.in_blocked8 = 1
    if out_blocked:                         # y leaves channel-blocked: the split-bf16 3x3 kernel (bias / PReLU epilogue), or plain 1x1
        ok3 = (pc.split and pc.ks == 3 and pc.cout % 8 == 0 and residual is None and act2 is None and act in (None, "prelu")
               and not split3x3_narrow(pc.cout) and not (in_add is not None and act is None))
        ok1 = not pc.split and pc.ks == 1 and pc.cout >= 33 and pc.cout % 8 == 0 and not up
        if not (ok3 or ok1):                # banks with 33..64 outputs on the fp32 MFMA kernel
            raise ValueError("conv2d: channel-blocked output is written by the split-bf16 3x3 kernel (bias / PReLU) and by the "
                             "direct 1x1 kernel with 40..64 output channels only")
        o.out_blocked8 = 1
    if out_stats is not None:
        if not conv_writes_stats(pc, act, residual, act2, out_blocked, in_add is not None):
            raise ValueError("conv2d: out_stats needs the split-bf16 3x3 kernel with an NCHW output and a bias / PReLU epilogue")
        if out_stats.dtype != torch.float64 or out_stats.numel() != 2 * pc.cout or not out_stats.is_cuda:
            raise ValueError("conv2d: out_stats must be a float64 [2*Cout] tensor on the HIP device")
        o.out_stats = out_stats.data_ptr()
    if out_sample_stats is not None:
        if not conv_writes_sample_stats(pc):
            raise ValueError("conv2d: out_sample_stats needs the few-channel split 7x7 kernel (a composed ConvNeXt bank with <= 8 inputs)")
        if out_sample_stats.dtype != torch.float64 or out_sample_stats.numel() != 2 * B or not out_sample_stats.is_cuda:
            raise ValueError("conv2d: out_sample_stats must be a float64 [2*B] tensor on the HIP device")
        o.out_sample_stats = out_sample_stats.data_ptr()
    rec = conv_event_sink
    if rec is not None:                    # bench.py: HIP events around selected launches, on the launch stream
        # the last field names the kernel instantiation the C side dispatches to (prologue / epilogue variant)
        key = (pc.ks, Cin, pc.cout, H, W, B, "%s|%s|%s|%s|%s" % ("pro" if (in_scale is not None or in_add is not None) else "",
                                                                 act or "", "res" if residual is not None else "", act2 or "",
                                                                 ("up" if up else "") + ("+split" if pc.split else "")),
               in_add is not None)
        if rec.want(key):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
    if walk:
        # 64 -> <= 48 channels, bias only: the conv phase of the layer kernel, persistent (csrc/conv_split_out.hip)
        check(L.cwfa_conv3x3_out_split_f32(_p(x), _p(pc.walk), _p(bias), _p(out), B, H, W, pc.cout, xbs, ybs, int(bool(in_blocked)),
                                           _stream()), "conv3x3_out_split")
    elif pc.split and pc.ks == 7:
        # the same kernel with a 3-pixel halo and 49 taps (bias-only epilogue, no prologue: what the ConvNeXt block needs)
        if act or act2 or residual is not None or in_scale is not None or in_add is not None:
            raise ValueError("conv2d: the split-bf16 7x7 kernel has a bias-only epilogue and no load-side prologue")
        check(L.cwfa_conv7x7_split_f32(_p(x), _p(pc.packed), _p(out), B, Cin, H, W, pc.cout, xbs, ybs, C.byref(o), _stream()),
              "conv7x7_split")
    elif pc.split and pc.ks == 3:
        if split3x3_narrow(pc.cout) and (in_scale is not None or in_add is not None):
            # the narrow tilings take no load-side prologue: one streaming pass materialises it (no such layer in CWFA's graphs)
            if (H * W) % 4 == 0:
                x = plane_affine(x, in_scale, in_shift, add=in_add)
            else:                               # odd plane sizes: per-channel affine pass(es) + an add pass
                if in_scale is not None:
                    if in_scale.numel() == Cin:
                        x = channel_affine(x, in_scale.reshape(-1), in_shift.reshape(-1))
                    else:
                        x = torch.cat([channel_affine(x[i:i + 1], in_scale.reshape(B, Cin)[i].contiguous(), in_shift.reshape(B, Cin)[i].contiguous())
                                       for i in range(B)], 0)
                if in_add is not None:
                    x = axpby(x.contiguous(), 1.0, in_add, 1.0)
            x, xbs = planes(x, "x")
            o.in_scale = o.in_shift = o.in_add = None
        # fp32-accurate conv on the bf16 pipe, the kernel splits x on the way into LDS (prologue included)
        check(L.cwfa_conv3x3_split_f32(_p(x), _p(pc.packed), _p(out), B, Cin, H, W, pc.cout, xbs, ybs, C.byref(o),
                                       _stream()), "conv3x3_split")
    elif pc.split:
        # fp32-accurate GEMM on the bf16 pipe: one pass splits x (with the load-side prologue) into three bf16 planes
        ws = torch.empty(L.cwfa_split_workspace_bytes(B, Cin, H * W), dtype=torch.uint8, device=x.device)
        per_sample = in_scale is not None and in_scale.numel() == B * Cin and B > 1
        check(L.cwfa_split_input_f32(_p(x), _p(ws), B, Cin, H * W, xbs, _p(in_scale), _p(in_shift), Cin if per_sample else 0,
                                     _p(in_add), in_add.stride(0) if in_add is not None else 0, _stream()), "split_input")
        o.in_scale = o.in_shift = o.in_add = None
        check(L.cwfa_conv_split_f32(_p(ws), _p(pc.packed), _p(out), B, Cin, H, W, pc.cout, pc.ks, ybs, C.byref(o), _stream()),
              "conv_split")
    else:
        check(L.cwfa_conv2d_f32(_p(x), _p(pc.packed), _p(out), B, Cin, H, W, pc.cout, pc.ks, xbs, ybs, C.byref(o),
                                _stream()), "conv2d")
    if rec is not None and rec.want(key):
        e1.record()
        rec.add(key, e0, e1)
    return out


def pack_couple_weight(w, bias):
    """Last convolution of a coupling sub-network, [2n,Cin,3,3] (+ bias [2n]): rows interleaved (cwfa_couple_rows) so that
    s_j and t_j of a pixel land in the same lane of the split-bf16 kernel, whose epilogue then applies the coupling."""
    L = _lib.lib()
    w = _dev(w, "weight").detach()
    n2, cin, ks, kw = w.shape
    if ks != 3 or kw != 3 or n2 % 2 or n2 // 2 > 64:
        raise ValueError(f"pack_couple_weight: a [2n,Cin,3,3] bank with n <= 64 is needed, got {tuple(w.shape)}")
    n = n2 // 2
    total = L.cwfa_couple_rows(n, None)
    rows_c = (C.c_int * total)()
    L.cwfa_couple_rows(n, rows_c)
    rows = torch.tensor(list(rows_c), dtype=torch.int64, device=w.device)
    live = (rows >= 0)
    wr = torch.zeros((total, cin, 3, 3), dtype=torch.float32, device=w.device)
    wr[live] = w[rows[live]]
    br = torch.zeros(total, dtype=torch.float32, device=w.device)
    if bias is not None:
        br[live] = _dev(bias, "bias").detach()[rows[live]]
    packed = torch.empty(L.cwfa_conv3x3_split_packed_bytes(total, cin), dtype=torch.uint8, device=w.device)
    check(L.cwfa_conv3x3_split_pack_f32(_p(wr), _p(packed), total, cin, _stream()), "conv3x3_split_pack (coupling bank)")
    pc = PackedConv(packed, n2, cin, 3, False, w._version, w.data_ptr(), split=True)
    pc.version1, pc.src_ptr1 = (bias._version, bias.data_ptr()) if bias is not None else (None, None)
    return pc, br


def conv3x3_couple(u, pc_bias, x, out, clamp_kind, clamp, pre_scale, rev, logdet=None, in_blocked=False):
    """out = coupling(x | s, t) with [s_raw | t] = conv3x3(u) + bias taken from the accumulators of the convolution (they never
    reach memory).  ``x`` / ``out``: the active half [B,n,H,W] (channel-slice views allowed; ``out`` may be ``x``)."""
    L = _lib.lib()
    pc, br = pc_bias
    u, ubs = planes(u, "u")
    B, Cin, H, W = u.shape
    n = pc.cout // 2
    if Cin != pc.cin:
        raise ValueError(f"conv3x3_couple: input has {Cin} channels, filter bank expects {pc.cin}")
    x2, xbs = planes(x, "x")
    o2, obs = planes(out, "out")
    if tuple(x.shape) != (B, n, H, W) or tuple(out.shape) != (B, n, H, W) or o2.data_ptr() != out.data_ptr():
        raise ValueError("conv3x3_couple: x / out must be [B,n,H,W] views with contiguous planes")
    cp = _lib.Couple()
    cp.x, cp.y, cp.x_bs, cp.y_bs, cp.n = x2.data_ptr(), out.data_ptr(), xbs, obs, n
    cp.clamp_kind, cp.clamp, cp.pre_scale, cp.rev = _lib.CLAMP[clamp_kind], float(clamp), float(pre_scale), int(bool(rev))
    if logdet is not None:
        cp.logdet = logdet.data_ptr()
    cp.in_blocked8 = int(bool(in_blocked))
    rec = conv_event_sink
    if rec is not None:
        key = (3, Cin, pc.cout, H, W, B, "||||couple+split", False)
        if rec.want(key):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
    check(L.cwfa_conv3x3_split_couple_f32(_p(u), _p(pc.packed), _p(br), B, Cin, H, W, ubs, C.byref(cp), _stream()),
          "conv3x3_split_couple")
    if rec is not None and rec.want(key):
        e1.record()
        rec.add(key, e0, e1)
    return out


BLOCKED_MAPS = True          # (tuning / ablation) False: the maps between the split-bf16 sub-network layers stay NCHW
SPLIT_7X7 = True             # (tuning / ablation) False: 7x7 convolutions stay on the fp32 MFMA kernel in split / bf16 precision
VIRTUAL_CAT = True           # (tuning / ablation) False: the input cat(half, condition) of a coupling sub-network is materialised
COUPLE_EPILOGUE = True       # (tuning / ablation) False: sub-networks write [s_raw | t] and a separate affine launch applies them


def couple_fused():
    """True when the coupling epilogue is available in the active precision mode (split / bf16: the split-bf16 3x3 kernel)."""
    return COUPLE_EPILOGUE and _split_bf16 >= 2


def split3x3_narrow(cout):
    """Banks the split-bf16 3x3 kernel runs on its narrow tilings (16 / 32 / 48 / 96 channels per block on the 16-row tile: no zero
    rows, more m-tiles per B fragment; csrc/conv_split3x3.hip: mpw_of / wm_of): no load-side prologue, NCHW output."""
    return cout <= 48 or 64 < cout <= 96


SPLIT_3X3_MIN_COUT = 1      # 3x3 banks with at least this many outputs take the split-bf16 kernel when "split_bf16" >= 2 (banks with <= 32 /
#                             <= 16 outputs: its narrow tilings of 32 / 16 channels per block; 33 = round 2's rule, those banks on fp32 Winograd)
SPLIT_3X3_NARROW_MAX = 16   # banks with <= this many outputs (and >= 29 inputs) take the 16-channel tiling of the split-bf16 kernel; 17..32
#                             outputs stay on the fp32 Winograd kernel.  Measured @512^2 (tools/small_conv_time.py, fp32 Winograd vs split): 64 -> 24:
#                             71 vs 76 us, 64 -> 12: 66 vs 58, 64 -> 6: 62 vs 56, 29 -> 12: 38 vs 32, 29 -> 6: 35 vs 31, 24 -> 24: 34 vs 39, 6 -> 6: 15 vs 29
#                             -- with so few MFMAs per step the per-step costs of the kernel (barrier, weight DMA, operand reads) decide
OUT_WALK = True             # (tuning / ablation) False: today's dispatch -- no bank takes the persistent output convolution.  Read when a bank is
#                             packed AND at every launch: switch it off at any time; switch it on before the banks are packed (or invalidate_packs())
OUT_WALK_MT = (1, 2, 3)     # widths, in 16-channel m-tiles, that take it (DESIGN.md section 9.1 lists a width that was sent back)


def out_walk_bank(cout, cin, ks, transposed=False):
    """Bank side of the rule for the persistent output convolution (cwfa_conv3x3_out_split_f32): split / bf16 / fp16 precision, a 3x3
    bank over exactly 64 inputs with at most 48 outputs -- the last convolution of a coupling sub-network."""
    return bool(OUT_WALK and _split_bf16 >= 2 and ks == 3 and not transposed and cin == 64 and 1 <= cout <= 48
                and (cout + 15) // 16 in OUT_WALK_MT)


def out_walk_selected(pc, H, W, act=None, prelu_alpha=None, residual=None, act2=None, in_scale=None, in_add=None, out_blocked=False,
                      cat=None, out_stats=None, out_sample_stats=None):
    """Launch side: conv2d(x, pc, bias=..., out=..., in_blocked=...) takes that kernel when the bank carries its image and the call
    has a bias-only epilogue, no load-side affine or add, no second source, an NCHW output and no statistics.  Everything else keeps
    its kernel."""
    return bool(OUT_WALK and getattr(pc, "walk", None) is not None and act is None and prelu_alpha is None
                and residual is None and act2 is None and in_scale is None and in_add is None and not out_blocked and cat is None
                and out_stats is None and out_sample_stats is None and 64 * H * W * 4 < 2 ** 31)


conv_event_sink = None      # object with want(key)->bool and add(key, start_event, end_event); set by bench.py only


def pack_1x1_panel(w):
    """[64,64,1,1] filter -> the lane-ordered A-operand image the fused sub-network layer consumes."""
    L = _lib.lib()
    w = _dev(w, "weight").detach().contiguous()
    if tuple(w.shape) != (64, 64, 1, 1):
        raise ValueError("pack_1x1_panel: the fused layer kernel is specialised for 64 channels")
    panel = torch.empty(4096, dtype=torch.float32, device=w.device)
    check(L.cwfa_subnet_pack1x1_f32(_p(w), _p(panel), _stream()), "subnet_pack1x1")
    return PackedConv(panel, 64, 64, 1, False, w._version, w.data_ptr())


def pack_split_layer_weight(w3, w1):
    """[64,64,3,3] and [64,64,1,1] filters -> the split-bf16 image of the fused layer (40 slices of three bf16 pieces)."""
    L = _lib.lib()
    w3 = _dev(w3, "weight").detach().contiguous()
    w1 = _dev(w1, "weight").detach().contiguous()
    if tuple(w3.shape) != (64, 64, 3, 3) or tuple(w1.shape) != (64, 64, 1, 1):
        raise ValueError("pack_split_layer_weight: 64x64x3x3 and 64x64x1x1 only")
    packed = torch.empty(L.cwfa_subnet_layer_split_packed_bytes(), dtype=torch.uint8, device=w3.device)
    check(L.cwfa_subnet_layer_split_pack_f32(_p(w3), _p(w1), _p(packed), _stream()), "subnet_layer_split_pack")
    pc = PackedConv(packed, 64, 64, 3, False, w3._version, w3.data_ptr(), split=True)
    pc.version1, pc.src_ptr1 = w1._version, w1.data_ptr()
    return pc


FIRST_LAYER_COMPOSED = True   # (tuning / ablation) False: the first layer of a sub-network runs like the other two (K = 9 x 64)
FIRST_LAYER_FUSED_X = True      # ... and its residual conv1x1(u) + b0 formed inside that launch (no first 1x1 launch, no first map in memory)


def pack_first_layer_weight(w0, b0, w3, w1, short=None):
    """The composed bank of a sub-network's FIRST layer (cwfa_subnet_layer_first_f32): conv3x3(conv1x1(u, w0) + b0, w3) =
    conv3x3(u | 1, w3c) with w3c[o][i][tap] = sum_m w3[o][m][tap] [w0 | b0][m][i] (formed in float64, rounded once), zero-padded to
    32 input channels; w0 [64,cin,1,1] with cin <= 31, b0 [64] or None, w3 [64,64,3,3], w1 [64,64,1,1]."""
    L = _lib.lib()
    w0, w3, w1 = _dev(w0, "w0").detach(), _dev(w3, "w3").detach(), _dev(w1, "w1").detach().contiguous()
    cin = w0.shape[1]
    if tuple(w0.shape) != (64, cin, 1, 1) or cin > 31 or tuple(w3.shape) != (64, 64, 3, 3) or tuple(w1.shape) != (64, 64, 1, 1):
        raise ValueError("pack_first_layer_weight: 64-channel layers with a 1x1 bank of <= 31 inputs in front only")
    w0p = torch.cat([w0.reshape(64, cin).double(), (b0.detach().double() if b0 is not None else torch.zeros(64, dtype=torch.float64, device=w0.device)).reshape(64, 1)], 1)
    wc = torch.einsum("omt,mi->oit", w3.double().reshape(64, 64, 9), w0p)
    w3c = torch.zeros((64, 32, 3, 3), dtype=torch.float32, device=w0.device)
    w3c[:, :cin + 1] = wc.reshape(64, cin + 1, 3, 3).to(torch.float32)
    w0c = torch.zeros((64, 32), dtype=torch.float32, device=w0.device)          # [W0 | b0 | 0]: the first map as a third k step of the 1x1 phase
    w0c[:, :cin + 1] = w0p.to(torch.float32)
    packed = torch.empty(L.cwfa_subnet_layer_first_packed_bytes(), dtype=torch.uint8, device=w0.device)
    # short form (u has one 16-channel chunk: five conv steps instead of nine) -- only launched with x = None (subnet_layer_first)
    short = (FIRST_LAYER_FUSED_X and cin + 1 <= 16) if short is None else bool(short)
    if short and cin + 1 > 16:
        raise ValueError("pack_first_layer_weight: the short form needs cin + 1 <= 16")
    check(L.cwfa_subnet_layer_first_pack_f32(_p(w3c), _p(w1), _p(w0c), int(short), _p(packed), _stream()), "subnet_layer_first_pack")
    pc = PackedConv(packed, 64, cin + 1, 3, False, w3._version, w3.data_ptr(), split=True)
    pc.short = short
    pc.version1, pc.src_ptr1 = w1._version, w1.data_ptr()
    return pc


CONVNEXT_COMPOSED = True      # (tuning / ablation) False: the 7x7 of a ConvNeXt block reads the 64-channel map of the 1x1 in front (K = 49 x 64)


def convnext_composed(c_in, c_out, biases=True):
    """True when a ConvNeXt block's 1x1 (c_in -> c_out) and 7x7 run as ONE composed few-channel 7x7 (pack_convnext_composed) in the
    active precision mode: split / bf16 / fp16, at most 16 inputs with the ones channel, at most 64 outputs, both biases present."""
    return bool(CONVNEXT_COMPOSED and SPLIT_7X7 and _split_bf16 >= 2 and c_in + 1 <= 16 and c_out <= 64 and biases)


def pack_convnext_composed(w0, b0, w7):
    """The composed bank of a ConvNeXt block's 7x7: conv7x7(conv1x1(x, w0) + b0, w7) = conv7x7(x | 1, wc) with wc[o][i][tap] =
    sum_m w7[o][m][tap] [w0 | b0][m][i] (formed in float64, rounded once; exact with zero padding: the padded ones channel carries no
    bias), zero-padded to 8 or 16 input channels for the few-channel forms of the split 7x7 kernel.  w0 [c,cin,1,1] with cin <= 15,
    b0 [c], w7 [cout <= 64,c,7,7].  The bank is launched on with_ones(x): ``cin`` + 1 channels."""
    L = _lib.lib()
    w0, b0, w7 = _dev(w0, "w0").detach(), _dev(b0, "b0").detach(), _dev(w7, "w7").detach()
    c, cin = w0.shape[0], w0.shape[1]
    cout = w7.shape[0]
    if tuple(w0.shape) != (c, cin, 1, 1) or cin + 1 > 16 or tuple(w7.shape) != (cout, c, 7, 7) or cout > 64 or tuple(b0.shape) != (c,):
        raise ValueError("pack_convnext_composed: a 1x1 bank with <= 15 inputs and a bias in front of a 7x7 bank with <= 64 outputs only")
    w0p = torch.cat([w0.reshape(c, cin).double(), b0.double().reshape(c, 1)], 1)
    wc = torch.einsum("omt,mi->oit", w7.double().reshape(cout, c, 49), w0p)
    cpad = 8 if cin + 1 <= 8 else 16
    w7c = torch.zeros((cout, cpad, 7, 7), dtype=torch.float32, device=w0.device)
    w7c[:, :cin + 1] = wc.reshape(cout, cin + 1, 7, 7).to(torch.float32)
    packed = torch.empty(L.cwfa_conv7x7_split_packed_bytes(cout, cpad), dtype=torch.uint8, device=w0.device)
    check(L.cwfa_conv7x7_split_pack_f32(_p(w7c), _p(packed), cout, cpad, _stream()), "conv7x7_split_pack (composed bank)")
    return PackedConv(packed, cout, cin + 1, 7, False, w7._version, w7.data_ptr(), split=True)


def subnet_layer_first(u1, x, pc, b3, b1, layout=0):
    """y = ELU(conv1x1(ELU(conv3x3'(u1) + b3)) + b1 + x): the first layer of a sub-network with its 3x3 composed with the 1x1 in
    front (pack_first_layer_weight).  ``u1``: the sub-network's input plus a constant-one channel [B, cin + 1 <= 32, H, W];
    ``x`` = conv1x1(u) + b0, the residual ([B,64,H,W]; ``layout`` bits as in subnet_layer), or None: the kernel then forms it itself
    as a third k step of its 1x1 phase (the first 1x1 launch of the sub-network and its map are never needed)."""
    L = _lib.lib()
    u1, ubs = planes(u1, "u1")
    B, Cu, H, W = u1.shape
    xbs = 0
    if x is not None:                       # (None: the kernel forms the first map itself from u1 and the packed [W0 | b0]: FIRST_LAYER_FUSED_X)
        x, xbs = planes(x, "x")
    if (x is not None and tuple(x.shape) != (B, 64, H, W)) or Cu != pc.cin:
        raise ValueError(f"subnet_layer_first: u1 {tuple(u1.shape)} / x {None if x is None else tuple(x.shape)} do not match the composed "
                         f"bank ({pc.cin} inputs)")
    short = bool(getattr(pc, "short", False))
    if short and x is not None:
        raise ValueError("subnet_layer_first: a short-form image (pack_first_layer_weight(short=True)) forms its first map itself: x must be None")
    out = torch.empty((B, 64, H, W), dtype=torch.float32, device=u1.device)
    rec = conv_event_sink
    if rec is not None:
        key = ("L", 16 if short else 32, 64, H, W, B, "layer1+split" if x is not None else "layer1x+split", False)
        if rec.want(key):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
    check(L.cwfa_subnet_layer_first_f32(_p(u1), _p(x), _p(pc.packed), _p(_dev(b3)), _p(_dev(b1)), _p(out), B, Cu, H, W, ubs, xbs,
                                        64 * H * W, int(layout) | (4 if short else 0), _stream()), "subnet_layer_first")
    if rec is not None and rec.want(key):
        e1.record()
        rec.add(key, e0, e1)
    return out


_ones_scope = None
_first_maps = None          # {id(sub-network): its first map x = conv1x1(u) + b0, channel-blocked} while a plan has them merged


class first_map_scope:
    """The first 1x1 convolutions of several sub-networks that read the SAME tensor (the five blocks of a CAT step all read the
    condition: coupling_layers.py:475-500, networks.py:621-623) as ONE launch with their banks stacked: the five 64-channel maps
    leave as consecutive channel-blocked chunks of one [B, 64 n, H, W] tensor."""

    def __init__(self, maps):
        self.maps = maps

    def __enter__(self):
        global _first_maps
        self.prev, _first_maps = _first_maps, self.maps
        return self

    def __exit__(self, *exc):
        global _first_maps
        _first_maps = self.prev
        return False


def first_map_of(net):
    return None if _first_maps is None else _first_maps.get(id(net))


class ones_channel_scope:
    """Within this scope ``with_ones(t)`` is computed once per tensor OBJECT (the five sub-networks of a CAT step read the same
    condition): cat(t, 1) through the strided plane-copy kernel."""

    def __enter__(self):
        global _ones_scope
        self.prev, _ones_scope = _ones_scope, {}
        return self

    def __exit__(self, *exc):
        global _ones_scope
        _ones_scope = self.prev
        return False


_ones_planes = {}


def ones_plane(B, H, W, device):
    """A constant [B,1,H,W] tensor of ones (read-only: the ones channel of the composed first layers), built once per shape."""
    key = (B, H, W, str(device))
    hit = _ones_planes.get(key)
    if hit is None:
        if len(_ones_planes) > 8:
            _ones_planes.clear()
        hit = _ones_planes[key] = torch.ones((B, 1, H, W), dtype=torch.float32, device=device)
    return hit


def with_ones(t):
    hit = _ones_scope.get(id(t)) if _ones_scope is not None else None
    if hit is not None and hit[0] is t:
        return hit[1]
    B, _, H, W = t.shape
    u1 = concat_channels([t, ones_plane(B, H, W, t.device)])
    if _ones_scope is not None:
        _ones_scope[id(t)] = (t, u1)
    return u1


def subnet_layer(x, pc3, b3, panel1, b1, want_hidden=False, layout=0):
    """y = ELU(conv1x1(ELU(conv3x3(x) + b3)) + b1 + x), 64 channels, one launch.  ``want_hidden`` (training forward):
    returns (y, h) with h = ELU(conv3x3(x) + b3), written by the same launch.  With ``pc3`` from
    pack_split_layer_weight (both banks in one split-bf16 image) ``panel1`` is unused; ``layout`` (split image only): bit 0 /
    bit 1 = input / output tensor is channel-blocked [B][8][H][W][8] (cwfa_subnet_layer_split_f32) -- the tensor object keeps
    the shape [B,64,H,W], only its memory order differs; the consumer must be told (layout bit 0, or ``in_blocked``)."""
    L = _lib.lib()
    x, xbs = planes(x, "x")
    B, Cc, H, W = x.shape
    if Cc != 64 or pc3.cin != 64 or pc3.cout != 64 or pc3.ks != 3:
        raise ValueError("subnet_layer: 64-channel 3x3 layers only")
    out = torch.empty((B, 64, H, W), dtype=torch.float32, device=x.device)
    if want_hidden:
        hid = torch.empty((B, 64, H, W), dtype=torch.float32, device=x.device)
        if pc3.split:
            if layout:
                raise ValueError("subnet_layer: the tape form keeps NCHW maps")
            check(L.cwfa_subnet_layer_split_tape_f32(_p(x), _p(pc3.packed), _p(_dev(b3)), _p(_dev(b1)), _p(out), _p(hid), B, H, W,
                                                     xbs, 64 * H * W, 64 * H * W, _stream()), "subnet_layer_split_tape")
            return out, hid
        check(L.cwfa_subnet_layer_tape_f32(_p(x), _p(pc3.packed), _p(_dev(b3)), _p(panel1.packed), _p(_dev(b1)), _p(out), _p(hid), B, H, W,
                                           xbs, 64 * H * W, 64 * H * W, _stream()), "subnet_layer_tape")
        return out, hid
    rec = conv_event_sink
    if rec is not None:
        key = ("L", 64, 64, H, W, B, "layer+split" if pc3.split else "layer", False)
        if rec.want(key):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
    if layout and not pc3.split:
        raise ValueError("subnet_layer: channel-blocked maps exist on the split-bf16 layer kernel only")
    if pc3.split:
        check(L.cwfa_subnet_layer_split_f32(_p(x), _p(pc3.packed), _p(_dev(b3)), _p(_dev(b1)), _p(out), B, H, W,
                                            xbs, 64 * H * W, int(layout), _stream()), "subnet_layer_split")
    else:
        check(L.cwfa_subnet_layer_f32(_p(x), _p(pc3.packed), _p(_dev(b3)), _p(panel1.packed), _p(_dev(b1)), _p(out), B, H, W,
                                      xbs, 64 * H * W, _stream()), "subnet_layer")
    if rec is not None and rec.want(key):
        e1.record()
        rec.add(key, e0, e1)
    return out


# ------------------------------------------------------------------------------------------------ backward of the sub-networks
_wgrad_ws = {}


def conv2d_wgrad(x, dy, ks, out=None, accumulate=False, bias_out=None, want_bias=False):
    """dW [Cout,Cin,ks,ks] of a stride-1 'same' convolution y = conv(x, W): sum over batch and pixels of dy (x) shifted x.
    With ``out`` and ``accumulate`` the result is added to ``out`` (a .grad buffer).  ``want_bias`` / ``bias_out``: also the
    bias gradient sum(dy) [Cout] from the same pass (returned as second value; accumulated like ``out``)."""
    L = _lib.lib()
    x, xbs = planes(x, "x")
    dy, dbs = planes(dy, "dy")
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    if tuple(dy.shape) != (B, Cout, H, W):
        raise ValueError(f"conv2d_wgrad: dy {tuple(dy.shape)} does not match x {tuple(x.shape)}")
    if out is None:
        out = torch.empty((Cout, Cin, ks, ks), dtype=torch.float32, device=x.device)
        accumulate = False
    elif tuple(out.shape) != (Cout, Cin, ks, ks) or not out.is_contiguous():
        raise ValueError("conv2d_wgrad: `out` must be a contiguous [Cout,Cin,ks,ks] tensor")
    if bias_out is None and want_bias:
        if accumulate:
            raise ValueError("conv2d_wgrad: accumulate needs an existing bias_out")
        bias_out = torch.empty(Cout, dtype=torch.float32, device=x.device)
    if bias_out is not None and (tuple(bias_out.shape) != (Cout,) or not bias_out.is_contiguous()):
        raise ValueError("conv2d_wgrad: `bias_out` must be a contiguous [Cout] tensor")
    nbytes = L.cwfa_conv2d_wgrad_workspace_bytes(B, Cin, H, W, Cout, ks)
    key = (x.device, torch.cuda.current_stream().cuda_stream)
    ws = _wgrad_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _wgrad_ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    check(L.cwfa_conv2d_wgrad_f32(_p(x), _p(dy), _p(out), _p(bias_out), _p(ws), B, Cin, H, W, Cout, ks, xbs, dbs,
                                  1.0 if accumulate else 0.0, _stream()), "conv2d_wgrad")
    return (out, bias_out) if bias_out is not None else out


def elu_bwd(g, a, add=None, out=None):
    """g * ELU'(q) from the activation output a = ELU(q) (+ add); may run in place on g."""
    L = _lib.lib()
    g, gbs = planes(g, "g")
    a, abs_ = planes(a, "a")
    B = g.shape[0]
    n = g[0].numel()
    if tuple(a.shape) != tuple(g.shape) or (add is not None and tuple(add.shape) != tuple(g.shape)):
        raise ValueError("elu_bwd: g, a (and add) differ in shape")
    addbs = 0
    if add is not None:
        add, addbs = planes(add, "add")
    if out is None:
        out = torch.empty(tuple(g.shape), dtype=torch.float32, device=g.device)
    o2, obs = planes(out, "out")
    if o2.data_ptr() != out.data_ptr():
        raise ValueError("elu_bwd: `out` must have contiguous planes")
    check(L.cwfa_elu_bwd_f32(_p(g), _p(a), _p(add), _p(out), B, n, gbs, abs_, addbs, obs, _stream()), "elu_bwd")
    return out


def plane_affine(x, scale=None, shift=None, add=None):
    """x * scale + shift (+ add) with [C] or [B,C] tables: a BatchNorm (x dropout mask) output as a tensor."""
    L = _lib.lib()
    x, xbs = planes(x, "x")
    B, Cc, H, W = x.shape
    per = 0
    if scale is not None:
        scale, shift = _dev(scale).contiguous(), _dev(shift).contiguous()
        if scale.numel() not in (Cc, B * Cc) or shift.numel() != scale.numel():
            raise ValueError("plane_affine: scale / shift must be [C] or [B,C]")
        per = int(scale.numel() == B * Cc and B > 1)
    abs_ = 0
    if add is not None:
        add, abs_ = planes(add, "add")
        if tuple(add.shape) != (B, Cc, H, W):       # (a centre-cropped skip of another size: the reference's `up + crop` raises too)
            raise ValueError(f"plane_affine: add {tuple(add.shape)} does not match x {(B, Cc, H, W)}")
    out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device)
    check(L.cwfa_plane_affine_f32(_p(x), _p(scale), _p(shift), per, _p(add), _p(out), B, Cc, H * W, xbs, abs_, Cc * H * W, _stream()),
          "plane_affine")
    return out


def bn_bwd_stats(g, y, mask_bc=None):
    """float64 [C,2]: (sum g*m, sum g*m*y) over (B,H,W)."""
    L = _lib.lib()
    g, gbs = planes(g, "g")
    y, ybs = planes(y, "y")
    B, Cc, H, W = g.shape
    if tuple(y.shape) != (B, Cc, H, W) or (mask_bc is not None and mask_bc.numel() != B * Cc):
        raise ValueError(f"bn_bwd_stats: g {tuple(g.shape)}, y {tuple(y.shape)} / mask do not match")
    st = torch.zeros(2 * Cc, dtype=torch.float64, device=g.device)
    check(L.cwfa_bn_bwd_stats_f32(_p(g), _p(y), _p(None if mask_bc is None else _dev(mask_bc).contiguous()), _p(st), B, Cc, H * W, gbs,
                                  ybs, _stream()), "bn_bwd_stats")
    return st.view(Cc, 2)


def bn_act_bwd(g, y, A, Bc, Cc_, alpha=None, dalpha=None, out=None):
    """(A*g + Bc + Cc*y) * PReLU'(y) (alpha None: identity activation); A is [C] or [B,C]."""
    L = _lib.lib()
    g, gbs = planes(g, "g")
    y, ybs = planes(y, "y")
    B, Cc, H, W = g.shape
    A = _dev(A).contiguous()
    if tuple(y.shape) != (B, Cc, H, W) or A.numel() not in (Cc, B * Cc) or Bc.numel() != Cc or Cc_.numel() != Cc:
        raise ValueError(f"bn_act_bwd: g {tuple(g.shape)}, y {tuple(y.shape)} or the coefficient tables do not match")
    per = int(A.numel() == B * Cc and B > 1)
    if out is None:
        out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=g.device)
    o2, obs = planes(out, "out")
    if o2.data_ptr() != out.data_ptr():
        raise ValueError("bn_act_bwd: `out` must have contiguous planes")
    check(L.cwfa_bn_act_bwd_f32(_p(g), _p(y), _p(A), per, _p(_dev(Bc).contiguous()), _p(_dev(Cc_).contiguous()),
                                _p(None if alpha is None else _dev(alpha)), _p(out), _p(dalpha), B, Cc, H * W, gbs, ybs, obs, _stream()),
          "bn_act_bwd")
    return out


def maxpool2_bwd(full, g_pool, g_skip=None):
    L = _lib.lib()
    full = _dev(full, "full").contiguous()
    g_pool = _dev(g_pool, "g_pool").contiguous()
    B, Cc, H, W = full.shape
    if tuple(g_pool.shape) != (B, Cc, H // 2, W // 2):
        raise ValueError(f"maxpool2_bwd: g_pool {tuple(g_pool.shape)} is not the 2x2-pooled shape of {tuple(full.shape)}")
    if g_skip is not None:
        g_skip = _dev(g_skip, "g_skip").contiguous()
        if tuple(g_skip.shape) != tuple(full.shape):
            raise ValueError("maxpool2_bwd: g_skip and full differ in shape")
    out = torch.empty_like(full)
    check(L.cwfa_maxpool2_bwd_f32(_p(full), _p(g_pool), _p(g_skip), _p(out), B, Cc, H, W, _stream()), "maxpool2_bwd")
    return out


def gelu_add(p, res=None):
    """GELU(p) + res (the unfused form of the ConvNeXt tail, kept for training: the backward needs p)."""
    L = _lib.lib()
    p = _dev(p, "p").contiguous()
    res = None if res is None else _dev(res).contiguous()
    if res is not None and tuple(res.shape) != tuple(p.shape):
        raise ValueError("gelu_add: p and res differ in shape")
    out = torch.empty_like(p)
    check(L.cwfa_gelu_f32(_p(p), _p(res), _p(out), p.numel(), 0, _stream()), "gelu")
    return out


def gelu_bwd(g, p):
    L = _lib.lib()
    p, g = _dev(p, "p").contiguous(), _dev(g, "g").contiguous()
    if tuple(g.shape) != tuple(p.shape):
        raise ValueError("gelu_bwd: g and p differ in shape")
    out = torch.empty_like(p)
    check(L.cwfa_gelu_f32(_p(p), _p(g), _p(out), p.numel(), 1, _stream()), "gelu_bwd")
    return out


def layernorm_bwd(g, v, weight, mean, invstd, dw, db):
    """dL/dv of a LayerNorm over (C,H,W); ``dw`` / ``db`` (shape of the affine) are accumulated in place."""
    L = _lib.lib()
    g, v = _dev(g, "g").contiguous(), _dev(v, "v").contiguous()
    B, n = v.shape[0], v[0].numel()
    if tuple(g.shape) != tuple(v.shape) or weight.numel() != n or mean.numel() != B or invstd.numel() != B or dw.numel() != n or db.numel() != n:
        raise ValueError("layernorm_bwd: operand shapes do not match")
    st = torch.zeros(2 * B, dtype=torch.float64, device=v.device)
    gv = torch.empty_like(v)
    check(L.cwfa_layernorm_bwd_f32(_p(g), _p(v), _p(_dev(weight).contiguous()), _p(_dev(mean).contiguous()), _p(_dev(invstd).contiguous()),
                                   _p(st), _p(gv), _p(dw), _p(db), B, n, _stream()), "layernorm_bwd")
    return gv


def attention_bwd(mean, w1, b1, w2, b2, m, g):
    """Backward of ``attention_combine(mean, ..., m, x)`` given g = dL/dout: (dL/dm, float64 [w1|b1|w2|b2] gradients); dL/dx = g."""
    L = _lib.lib()
    mean, m, g = _dev(mean).contiguous(), _dev(m).contiguous(), _dev(g).contiguous()
    if tuple(m.shape) != tuple(mean.shape) or tuple(g.shape) != tuple(mean.shape):
        raise ValueError("attention_bwd: mean, m and g differ in shape")
    B, Cc = mean.shape[:2]
    HW = mean[0, 0].numel()
    gm = torch.empty_like(m)
    pg = torch.zeros(Cc * Cc * 3 + Cc + Cc * Cc + Cc, dtype=torch.float64, device=mean.device)
    check(L.cwfa_attention_bwd_f32(_p(mean), _p(_dev(w1).contiguous()), _p(_dev(b1)), _p(_dev(w2).contiguous()), _p(_dev(b2)), _p(m),
                                   _p(g), _p(gm), _p(pg), B, Cc, HW, _stream()), "attention_bwd")
    return gm, pg


def prelu_bwd(g, o, alpha, dalpha=None, out=None):
    """g * PReLU'(q) from the activation output o (single alpha > 0); ``dalpha`` (float64[1]) accumulates sum g*min(q,0)."""
    L = _lib.lib()
    g, gbs = planes(g, "g")
    o, obs = planes(o, "o")
    if tuple(o.shape) != tuple(g.shape):
        raise ValueError("prelu_bwd: g and o differ in shape")
    B, n = g.shape[0], g[0].numel()
    if out is None:
        out = torch.empty(tuple(g.shape), dtype=torch.float32, device=g.device)
    o2, ybs = planes(out, "out")
    if o2.data_ptr() != out.data_ptr():
        raise ValueError("prelu_bwd: `out` must have contiguous planes")
    check(L.cwfa_prelu_bwd_f32(_p(g), _p(o), _p(_dev(alpha)), _p(out), _p(dalpha), B, n, gbs, obs, ybs, _stream()), "prelu_bwd")
    return out


def conv3d_1k1_backward(x, dy, w1, b1, alpha, w2, want_input_grad=True):
    """Backward of ``conv3d_1k1`` (y = W2 * PReLU(W1 * x + b1) + b2): returns (dx or None, dW1, db1, dW2, db2, dalpha[float64 1])."""
    L = _lib.lib()
    x = _dev(x, "x").contiguous()
    dy = _dev(dy, "dy").contiguous()
    B, D, H, W = x.shape
    K = w1.shape[0]
    w1c, w2c = _dev(w1).detach().contiguous(), _dev(w2).detach().contiguous()
    st = _stream()
    q = torch.empty((B, K, D, H, W), dtype=torch.float32, device=x.device)
    m = torch.empty_like(q)
    dalpha = torch.zeros(1, dtype=torch.float64, device=x.device)
    ws = torch.empty(L.cwfa_conv3d_wgrad_workspace_bytes(B, D, H, W), dtype=torch.uint8, device=x.device)
    g2 = torch.empty(32, 32, dtype=torch.float32, device=x.device)
    g1 = torch.empty(32, 32, dtype=torch.float32, device=x.device)
    check(L.cwfa_conv3d_hidden_fwd_f32(_p(x), _p(w1c), _p(_dev(b1)), _p(q), B, D, H, W, K, st), "conv3d_hidden_fwd")
    check(L.cwfa_conv3d_wgrad_f32(_p(q), _p(dy), _p(_dev(alpha)), _p(g2), _p(ws), B, D, H, W, K, -1, 0, 0.0, st), "conv3d_wgrad")
    check(L.cwfa_conv3d_hidden_bwd_f32(_p(dy), _p(w2c), _p(q), _p(_dev(alpha)), _p(m), _p(dalpha), B, D, H, W, K, st), "conv3d_hidden_bwd")
    check(L.cwfa_conv3d_wgrad_f32(_p(m), _p(x), None, _p(g1), _p(ws), B, D, H, W, K, 1, 1, 0.0, st), "conv3d_wgrad")
    dx = None
    if want_input_grad:
        dx = torch.empty_like(x)
        check(L.cwfa_conv3d_input_bwd_f32(_p(m), _p(w1c), _p(dx), B, D, H, W, K, st), "conv3d_input_bwd")
    dW1 = g1[:K, :27].reshape(K, 1, 3, 3, 3).contiguous()
    db1 = g1[:K, 27].contiguous()
    dW2 = g2[:K, :27].reshape(1, K, 3, 3, 3).contiguous()
    db2 = sample_stats(dy.reshape(1, -1, 1, 1))[0:1].to(torch.float32)
    return dx, dW1, db1, dW2, db2, dalpha


SPLIT_CONV3D = True          # (tuning / ablation) False: the fused Conv3d of the condition nets stays on the fp32 MFMA kernel in split / bf16 precision


def conv3d_1k1(x, w1, b1, alpha, w2, b2):
    """Conv3d(1->K) -> PReLU -> Conv3d(K->1) over the (H, W, depth) volume of a [B,D,H,W] tensor (networks.py:221-225,239), one
    launch; in split / bf16 precision on the bf16 matrix cores (cwfa_conv3d_1k1_split_f32), else fp32 MFMA."""
    L = _lib.lib()
    x = _dev(x, "x").contiguous()
    B, D, H, W = x.shape
    K = w1.shape[0]
    out = torch.empty_like(x)
    if SPLIT_CONV3D and _split_bf16 >= 2 and K <= 32 and (D + 4) * H * W * 4 < 2 ** 31:
        check(L.cwfa_conv3d_1k1_split_f32(_p(x), _p(_dev(w1).contiguous()), _p(_dev(b1)), _p(_dev(alpha)), _p(_dev(w2).contiguous()),
                                          _p(_dev(b2)), _p(out), B, D, H, W, K, _stream()), "conv3d_1k1_split")
        return out
    check(L.cwfa_conv3d_1k1_f32(_p(x), _p(_dev(w1).contiguous()), _p(_dev(b1)), _p(_dev(alpha)), _p(_dev(w2).contiguous()),
                                _p(_dev(b2)), _p(out), B, D, H, W, K, _stream()), "conv3d_1k1")
    return out


# ------------------------------------------------------------------------------------------------ LRNN helpers
def channel_stats(x, out=None):
    """double[2*C]: per-channel (sum, sumsq) over (B,H,W).  ``out``: a ZEROED float64[2*C] buffer to add into (bn_finish clears
    it again) instead of a fresh one."""
    L = _lib.lib()
    x, xbs = planes(x, "x")
    B, Cc, H, W = x.shape
    st = out if out is not None else torch.zeros(2 * Cc, dtype=torch.float64, device=x.device)
    check(L.cwfa_channel_stats_f32(_p(x), _p(st), B, Cc, H * W, xbs, _stream()), "channel_stats")
    return st


def bn_running_update(stats, count, momentum, running_mean, running_var, num_batches_tracked=None):
    """nn.BatchNorm2d's train-mode update of its buffers from channel_stats() sums, in place, one launch."""
    L = _lib.lib()
    check(L.cwfa_bn_running_update_f32(_p(stats), float(count), float(momentum), _p(_dev(running_mean)), _p(_dev(running_var)),
                                       _p(num_batches_tracked), running_mean.numel(), _stream()), "bn_running_update")


def bn_fold(C_, weight=None, bias=None, eps=1e-5, stats=None, count=0.0, running_mean=None, running_var=None,
            mask_bc=None):
    """(scale, shift) of a BatchNorm (batch or running statistics), optionally times a per-(sample,channel) mask."""
    L = _lib.lib()
    ref = next(t for t in (weight, stats, running_mean, mask_bc) if t is not None)
    B = 0
    n = C_
    if mask_bc is not None:
        mask_bc = _dev(mask_bc, "mask").contiguous()
        B = mask_bc.numel() // C_
        n = B * C_
    scale = torch.empty(n, dtype=torch.float32, device=ref.device)
    shift = torch.empty(n, dtype=torch.float32, device=ref.device)
    check(L.cwfa_bn_fold_f32(_p(stats), float(count), _p(running_mean), _p(running_var), _p(weight), _p(bias),
                             float(eps), _p(mask_bc), B, _p(scale), _p(shift), C_, _stream()), "bn_fold")
    return scale, shift


def bn_finish(C_, weight=None, bias=None, eps=1e-5, stats=None, count=0.0, running_mean=None, running_var=None, momentum=None,
              num_batches_tracked=None, mask_bc=None, mask_u=None, drop_p=0.0, zero_stats=False):
    """bn_fold + bn_running_update (``momentum`` not None) in ONE launch; the dropout factor may be given as the raw uniform draw
    ``mask_u`` [B,C] with ``drop_p`` (m = (u >= p) / (1 - p), exactly F.dropout2d's keep / (1 - p)); ``zero_stats`` clears the
    statistics buffer for its next accumulation."""
    L = _lib.lib()
    ref = next(t for t in (weight, stats, running_mean, mask_bc, mask_u) if t is not None)
    B, n = 0, C_
    mk = mask_bc if mask_bc is not None else mask_u
    if mk is not None:
        mk = _dev(mk, "mask").contiguous()
        B = mk.numel() // C_
        n = B * C_
    scale = torch.empty(n, dtype=torch.float32, device=ref.device)
    shift = torch.empty(n, dtype=torch.float32, device=ref.device)
    upd = momentum is not None and stats is not None and running_mean is not None
    check(L.cwfa_bn_finish_f32(_p(stats), float(count), _p(running_mean), _p(running_var), _p(num_batches_tracked),
                               float(momentum or 0.0), int(upd), _p(weight), _p(bias), float(eps), _p(mk if mask_bc is not None else None),
                               _p(mk if mask_u is not None else None), float(drop_p), float(1.0 - drop_p), B, _p(scale), _p(shift), C_,
                               int(bool(zero_stats)), _stream()), "bn_finish")
    return scale, shift


def maxpool(x, Ho, Wo, scale=None, shift=None, want_full=False):
    L = _lib.lib()
    x = _dev(x, "x").contiguous()
    B, Cc, H, W = x.shape
    for t in (scale, shift):
        if t is not None and t.numel() != Cc:
            raise ValueError("maxpool: the load-side affine must be a [C] table")
    y = torch.empty((B, Cc, Ho, Wo), dtype=x.dtype, device=x.device)
    full = torch.empty_like(x) if want_full else None
    check(L.cwfa_maxpool_f32(_p(x), _p(y), _p(full), _p(scale), _p(shift), B, Cc, H, W, Ho, Wo, _stream()), "maxpool")
    return (y, full) if want_full else y


def sample_stats(x):
    L = _lib.lib()
    x = _dev(x, "x").contiguous()
    B = x.shape[0]
    st = torch.zeros(2 * B, dtype=torch.float64, device=x.device)
    check(L.cwfa_sample_stats_f32(_p(x), _p(st), B, x[0].numel(), _stream()), "sample_stats")
    return st


def layernorm_apply(x, stats, weight, bias, eps):
    L = _lib.lib()
    x = _dev(x, "x").contiguous()
    if stats.numel() != 2 * x.shape[0] or weight.numel() != x[0].numel() or bias.numel() != x[0].numel():
        raise ValueError("layernorm_apply: statistics / affine do not match x")
    out = torch.empty_like(x)
    check(L.cwfa_layernorm_apply_f32(_p(x), _p(stats), _p(weight), _p(bias), float(eps), _p(out), x.shape[0],
                                     x[0].numel(), _stream()), "layernorm_apply")
    return out


CONVNEXT_TAIL_FUSED = True        # (tuning / ablation) False: ConvNeXt.forward runs layernorm_apply, scale_channels and the fp32 1x1 launch
CONVNEXT_RESIDUAL_FUSED = True    # (tuning / ablation) False: the composed block still writes u = conv1x1(x) + b0 for the tail to read


def convnext_tail(v, stats, ln_weight, ln_bias, eps, w1, b1, u=None, gate=None, x=None, w0=None, b0=None, out=None):
    """The tail of a ConvNeXt block in one launch: GELU(conv1x1(LayerNorm(v), w1) + b1) + gate[b] * u, bit for bit what
    layernorm_apply -> scale_channels -> conv2d(act="gelu", residual=) give.  v [B,C <= 64,H,W]; stats: float64 [2B] (sample_stats,
    or conv2d(out_sample_stats=)); w1 [C,C,1,1]; gate: [B] or None (= 1).  The residual is ``u`` [B,C,H,W], or with ``u`` None it is
    formed in the launch from the block input ``x`` [B,c_in <= 8,H,W] as conv1x1(x, w0) + b0 (the fp32 1x1 kernel's bits)."""
    L = _lib.lib()
    v, vbs = planes(v, "v")
    B, Cc, H, W = v.shape
    HW = H * W
    if stats.dtype != torch.float64 or stats.numel() != 2 * B or not stats.is_cuda:
        raise ValueError("convnext_tail: stats must be a float64 [2*B] tensor on the HIP device")
    ln_weight, ln_bias = _dev(ln_weight, "ln_weight").contiguous(), _dev(ln_bias, "ln_bias").contiguous()
    w1 = _dev(w1, "w1").detach().contiguous()
    if Cc > 64 or ln_weight.numel() != Cc * HW or ln_bias.numel() != Cc * HW or w1.numel() != Cc * Cc:
        raise ValueError("convnext_tail: C <= 64, LayerNorm tables of C*H*W values and a [C,C,1,1] bank are needed")
    if b1 is not None and _dev(b1, "b1").numel() != Cc:
        raise ValueError("convnext_tail: b1 must hold C values")
    if (u is None) == (x is None):
        raise ValueError("convnext_tail: pass the residual u, or the block input x it is formed from")
    ubs = xbs = cin = 0
    if u is not None:
        u, ubs = planes(u, "u")
        if tuple(u.shape) != (B, Cc, H, W):
            raise ValueError(f"convnext_tail: residual {tuple(u.shape)} != {(B, Cc, H, W)}")
    else:
        x, xbs = planes(x, "x")
        cin = x.shape[1]
        w0 = _dev(w0, "w0").detach().contiguous()
        if tuple(x.shape) != (B, cin, H, W) or cin > 8 or w0.numel() != Cc * cin or (b0 is not None and _dev(b0, "b0").numel() != Cc):
            raise ValueError("convnext_tail: x [B,c_in <= 8,H,W] with w0 [C,c_in,1,1] and b0 [C] is needed")
    if gate is not None:
        gate = _dev(gate, "gate").reshape(-1).contiguous()
        if gate.numel() != B:
            raise ValueError("convnext_tail: gate must hold one factor per sample")
    if out is None:
        out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=v.device)
        ybs = Cc * HW
    else:
        out_c, ybs = planes(out, "out")
        if tuple(out.shape) != (B, Cc, H, W) or out_c.data_ptr() != out.data_ptr():
            raise ValueError("convnext_tail: `out` must be [B,C,H,W] with contiguous planes")
    check(L.cwfa_convnext_tail_f32(_p(v), _p(stats), _p(ln_weight), _p(ln_bias), float(eps), _p(w1), _p(b1), _p(u), _p(gate), _p(x),
                                   _p(w0), _p(b0), cin, _p(out), B, Cc, HW, vbs, ubs, xbs, ybs, _stream()), "convnext_tail")
    return out


def attention_combine(mean, w1, b1, w2, b2, m=None, x=None):
    L = _lib.lib()
    mean = _dev(mean, "mean").contiguous()
    B, Cc = mean.shape[:2]
    HW = mean[0, 0].numel()
    out = torch.empty_like(mean)
    m = None if m is None else _dev(m).contiguous()
    x = None if x is None else _dev(x).contiguous()
    for t in (m, x):
        if t is not None and tuple(t.shape) != tuple(mean.shape):
            raise ValueError("attention_combine: mean, m and x must share one shape")
    if w1.numel() != Cc * Cc * 3 or b1.numel() != Cc or w2.numel() != Cc * Cc or b2.numel() != Cc:
        raise ValueError("attention_combine: the Conv1d banks do not match the channel count")
    check(L.cwfa_attention_combine_f32(_p(mean), _p(_dev(w1).contiguous()), _p(_dev(b1)), _p(_dev(w2).contiguous()),
                                       _p(_dev(b2)), _p(m), _p(x), _p(out), B, Cc, HW, _stream()), "attention_combine")
    return out


def scale_channels(x, scale_bc):
    L = _lib.lib()
    x = _dev(x, "x").contiguous()
    B, Cc = x.shape[:2]
    if scale_bc.numel() != B * Cc:
        raise ValueError(f"scale_channels: the table must hold B*C = {B * Cc} factors")
    out = torch.empty_like(x)
    check(L.cwfa_scale_channels_f32(_p(x), _p(_dev(scale_bc).contiguous()), _p(out), B, Cc, x[0, 0].numel(), _stream()),
          "scale_channels")
    return out


def axpby(x, a, z=None, b=0.0):
    L = _lib.lib()
    x = _dev(x, "x").contiguous()
    z = None if z is None else _dev(z).contiguous()
    if z is not None and z.numel() != x.numel():
        raise ValueError("axpby: x and z differ in size")
    out = torch.empty_like(x)
    check(L.cwfa_axpby_f32(_p(x), _p(z), float(a), float(b), _p(out), x.numel(), _stream()), "axpby")
    return out


def extract_views(image, coords_yx, subimage_shape, mean=0.0, std=1.0):
    """XLFMDatasetFull.extract_views (XLFMDataset.py:212-242) + (v - mean) / std (CWFA.py:796-797) in one launch.
    image [B,1,Hs,Ws] fp32 on the HIP device; coords_yx: n x 2 integers (row, column) of the lenslet centres."""
    L = _lib.lib()
    image = _dev(image, "image")
    if image.dim() != 4 or image.shape[1] != 1:
        raise ValueError(f"extract_views: image must be [B,1,H,W], got {tuple(image.shape)}")
    if image.dtype != torch.float32:
        raise TypeError("extract_views: fp32 images only")
    image = image if image[0].is_contiguous() else image.contiguous()
    B, _, Hs, Ws = image.shape
    co = torch.as_tensor(coords_yx, dtype=torch.int32).reshape(-1, 2)
    sh, sw = int(subimage_shape[0]), int(subimage_shape[1])
    ys, xs = co[:, 0], co[:, 1]
    if len(co) and (bool(((torch.minimum(ys + sh // 2, torch.tensor(Hs)) - torch.clamp(ys - sh // 2, min=0)) <= 0).any()) or
                    bool(((torch.minimum(xs + sw // 2, torch.tensor(Ws)) - torch.clamp(xs - sw // 2, min=0)) <= 0).any())):
        raise ValueError("extract_views: a lenslet window lies outside the image")    # the reference raises on the empty patch
    cod = co.contiguous().to(image.device)
    out = torch.empty((B, len(co), sh, sw), dtype=torch.float32, device=image.device)
    check(L.cwfa_extract_views_f32(_p(image), _p(cod), _p(out), B, Hs, Ws, len(co), sh, sw, float(mean), float(std),
                                   image.stride(0), _stream()), "extract_views")
    return out


_split_bf16 = 0
_precision = "fp32"      # the mode of the last set_precision()
_pack_epoch = 0


def single_product():
    """True in the "bf16" and "fp16" modes: the split kernels with ONE product of plain 16-bit operands (BASELINE.json configs[4]);
    the two modes route every convolution alike and differ only in the operand format."""
    return _precision in ("bf16", "fp16")


def pack_epoch():
    """Generation counter of the packing-relevant options; a cached PackedConv with another epoch must be rebuilt."""
    return _pack_epoch


def invalidate_packs():
    """Drop every cached kernel-layout image (filter banks, packed biases, composed chain tables): they are keyed on
    ``tensor._version`` / ``data_ptr()``, which an in-place write through ``.data`` (``m.bias.data *= 0.1``,
    ``nn.init.*_(m.weight.data)`` -- the reference's own initialisers, networks.py:19-62) does NOT change.  The initialisers and
    reset helpers of cwfa_amd.networks call this; call it yourself after any other ``.data`` edit of a parameter that has
    already been used in a forward pass."""
    global _pack_epoch
    _pack_epoch += 1


WINOGRAD_2D_DEFAULT = 512     # library default of the "winograd_2d" option (output-channel threshold of the 2-D kernel)


def set_option(name, value):
    """Process-wide tuning option (see cwfa_set_option in include/cwfa_hip.h).  Filter banks packed before a change of
    "winograd_min_cout" / "winograd_2d" / "split_bf16" must be re-packed.
    "split_bf16" (host-side switch, default 0): 1x1 convolutions and ConvTranspose2d(k2,s2) with >= 128 output channels
    run as an fp32-accurate GEMM on the bf16 matrix pipe (cwfa_split_input_f32 + cwfa_conv_split_f32)."""
    global _split_bf16, _pack_epoch
    _pack_epoch += 1
    if name == "split_bf16":          # 0 off, 1: 1x1 / transposed convs, 2: also 3x3 convs and the fused 64-channel layers
        _split_bf16 = int(value)
        return
    check(_lib.lib().cwfa_set_option(name.encode(), int(value)), "set_option")


PRECISIONS = ("fp32", "split_bf16", "bf16", "fp16")


def set_precision(mode):
    """"fp32" (library default: plain fp32 MFMA / Winograd kernels) | "split_bf16" (the benchmark's arithmetic, fp32-equivalent:
    three bf16 pieces per operand, six products, fp32 accumulation) | "bf16" (BASELINE.json configs[4]: the same kernels with ONE
    product, i.e. plain bf16 operands and fp32 accumulation) | "fp16" (the same as "bf16" with fp16 operands, rounded to nearest
    even as torch's .half(): the arithmetic of the reference's CUDA autocast).  The split / bf16 / fp16 kernels
    take: 1x1 and transposed convolutions with >= 128 outputs, 3x3 convolutions with >= SPLIT_3X3_MIN_COUT outputs, the 64-channel
    fused layers, the Conv3d of the condition nets; wavelets, couplings, permutations and the remaining small convolutions stay fp32.
    Weight gradients (training) take the split arithmetic in "split_bf16" and plain bf16 operands in "bf16" and "fp16"."""
    if mode not in PRECISIONS:
        raise ValueError(f"set_precision: unknown mode {mode!r}")
    global _precision
    _precision = mode
    set_option("split_operand", 0)                              # (first: (6 products, fp16) is not a valid pair)
    set_option("split_products", 1 if single_product() else 6)
    if mode == "fp16":
        set_option("split_operand", 1)
    set_option("split_bf16", 0 if mode == "fp32" else 2)
    set_option("wgrad_split", 0 if mode == "fp32" else 1)        # training: 3x3 weight gradients in the same arithmetic (csrc/conv_bwd.hip)


def copy_channels(src, dst):
    """dst[...] = src for [B,c,H,W] views with contiguous planes (channel slices of NCHW tensors): one strided plane-copy launch."""
    L = _lib.lib()
    s_, sbs = planes(src, "src")
    d_, dbs = planes(dst, "dst")
    if d_.data_ptr() != dst.data_ptr() or tuple(src.shape) != tuple(dst.shape):
        raise ValueError("copy_channels: dst must be a [B,c,H,W] view with contiguous planes of src's shape")
    B, Cc, H, W = s_.shape
    check(L.cwfa_channel_affine_f32(_p(s_), _p(dst), None, None, 0, None, None, B, Cc, H * W, sbs, dbs, _stream()), "copy_channels")
    return dst


def concat_channels(parts):
    """torch.cat(parts, 1) through the strided plane-copy kernel (coupling_layers.py:74-87 materialise this too)."""
    L = _lib.lib()
    parts = [planes(t, "part") for t in parts]
    B, _, H, W = parts[0][0].shape
    Ct = sum(t.shape[1] for t, _ in parts)
    out = torch.empty((B, Ct, H, W), dtype=torch.float32, device=parts[0][0].device)
    c0 = 0
    for t, bs in parts:
        if t.shape[0] != B or t.shape[2:] != (H, W):
            raise ValueError("concat_channels: shape mismatch")
        check(L.cwfa_channel_affine_f32(_p(t), C.c_void_p(out.data_ptr() + 4 * c0 * H * W), None, None, 0, None, None, B,
                                        t.shape[1], H * W, bs, Ct * H * W, _stream()), "concat_channels")
        c0 += t.shape[1]
    return out


# ------------------------------------------------------------------------------------------------ evaluation pass
def eval_affine(step, mean, std):
    """The de-normalisation the evaluation kernels apply on load: v -> (v * 2^-step) * std - mean (CWFA.py:112-117).  mean and std
    may be numbers or one-element tensors; they are rounded to fp32 like the reference's scalar operands."""
    a = _lib.EvalAffine()
    a.enabled, a.scale = 1, 2.0 ** -int(step)
    a.std = float(torch.as_tensor(std, dtype=torch.float32).reshape(()).cpu())
    a.mean = float(torch.as_tensor(mean, dtype=torch.float32).reshape(()).cpu())
    return a


def _aff(a):
    return None if a is None else C.byref(a)


def _pair(a, b, what):
    a, a_bs = planes(a, what)
    b_bs = 0
    if b is not None:
        b, b_bs = planes(b, what)
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"{what}: the two tensors differ in shape: {tuple(a.shape)} vs {tuple(b.shape)}")
    return a, a_bs, b, b_bs


def volume_extrema(a, b=None, affine=None):
    """Per sample of [B,D,H,W]: float32 [B, 12] = (min, max, min|.|, max|.|) of a, the same of b, (min, max) of |a - b|, 0, 0.
    Exact.  Inputs are assumed finite."""
    L = _lib.lib()
    a, a_bs, b, b_bs = _pair(a, b, "volume_extrema")
    B = a.shape[0]
    out = torch.zeros(B, _lib.EXTREMA_STRIDE, dtype=torch.float32, device=a.device)
    ws = torch.empty(max(1, B * L.cwfa_eval_splits(B, a[0].numel()) * 10), dtype=torch.float32, device=a.device)
    check(L.cwfa_volume_extrema_f32(_p(a), _p(b), _p(out), _p(ws), B, a[0].numel(), a_bs, b_bs, _aff(affine), _stream()), "volume_extrema")
    return out


def volume_metrics(pred, gt, thr=float("-inf"), affine=None, pred_offset=0.0, gt_offset=0.0):
    """Per sample: float64 [B, 4] = (sum (g-p)^2, sum g, sum |g - p~|, #{p < thr}), p~ = p with every p < thr set to 0.
    One pass, float64 sums added in a fixed order.  Inputs are assumed finite."""
    L = _lib.lib()
    pred, p_bs, gt, g_bs = _pair(pred, gt, "volume_metrics")
    B = pred.shape[0]
    out = torch.zeros(B, 4, dtype=torch.float64, device=pred.device)
    ws = torch.empty(max(1, B * L.cwfa_eval_splits(B, pred[0].numel()) * 4), dtype=torch.float64, device=pred.device)
    check(L.cwfa_volume_metrics_f32(_p(pred), _p(gt), _p(out), _p(ws), B, pred[0].numel(), p_bs, g_bs, _aff(affine),
                                    float(pred_offset), float(gt_offset), float(thr), _stream()), "volume_metrics")
    return out


def mip3(a, b=None, triple=False, affine=None, post=None):
    """The three maximum projections of |a| (or |a - b|) of [B,D,H,W] in one read: (over depth [B,H,W], over H [B,W,D],
    over W [B,H,D], min [B]).  ``triple``: those of |a|, |b| and |a - b| in the same read, every output with a leading [3].
    Bit-exact and bitwise reproducible.  Inputs are assumed finite."""
    L = _lib.lib()
    a, a_bs, b, b_bs = _pair(a, b, "mip3")
    B, D, H, W = a.shape
    lead = (3, B) if triple else (B,)
    dev = a.device
    zp = torch.empty(*lead, H, W, dtype=torch.float32, device=dev)
    xp = torch.empty(*lead, W, D, dtype=torch.float32, device=dev)
    yp = torch.empty(*lead, H, D, dtype=torch.float32, device=dev)
    gmin = torch.empty(*lead, dtype=torch.float32, device=dev)
    check(L.cwfa_mip3_f32(_p(a), _p(b), _p(zp), _p(xp), _p(yp), _p(gmin), B, D, H, W, a_bs, b_bs, int(bool(triple)), _aff(affine),
                          None if post is None else C.byref(post), _stream()), "mip3")
    return zp, xp, yp, gmin


def projection_compose(zp, xp, yp, fill, depth_scale=2, border=2, scale_bars=False):
    """The composite image of utils.py:305-325 from the projections of ``mip3``: [B, H + D*depth_scale + border, W + ...].
    ``fill``: one-element device tensor (the reference's ``z_projection.min()``)."""
    L = _lib.lib()
    zp, xp, yp, fill = (_dev(t).contiguous() for t in (zp, xp, yp, fill))
    B, H, W = zp.shape
    D = xp.shape[2]
    if tuple(xp.shape) != (B, W, D) or tuple(yp.shape) != (B, H, D) or fill.numel() != 1:
        raise ValueError("projection_compose: projections of different volumes")
    side = D * int(depth_scale) + int(border)
    out = torch.empty(B, H + side, W + side, dtype=torch.float32, device=zp.device)
    check(L.cwfa_projection_compose_f32(_p(zp), _p(xp), _p(yp), _p(fill), _p(out), B, D, H, W, int(depth_scale), int(border),
                                        int(bool(scale_bars)), _stream()), "projection_compose")
    return out


def roi_means(stack, boxes):
    """float64 [N, T]: the mean of stack[t, z0:z1, y0:y1, x0:x1] for every box (z0,z1,y0,y1,x0,x1) of the integer [N,6] host table
    (inside the volume; an empty box gives NaN).  stack: [T,D,H,W]."""
    import numpy as np
    L = _lib.lib()
    stack, t_bs = planes(stack, "roi_means")
    T, D, H, W = stack.shape
    bx = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 6))
    out = torch.empty(len(bx), T, dtype=torch.float64, device=stack.device)
    check(L.cwfa_roi_means_f32(_p(stack), C.c_void_p(bx.ctypes.data), _p(out), T, D, H, W, len(bx), t_bs, _stream()), "roi_means")
    return out


def select_positive(x, k=-1):
    """(value float32[1], count int64[1]) on the device: the k-th smallest (k = 0 ..) of the strictly positive elements of x
    ([B,D,H,W]); k = -1: their lower median (torch's ``median``).  Exact (radix selection, 64-bit counters: up to 2^45 elements per
    sample); NaN if k >= count.  Inputs are assumed finite."""
    L = _lib.lib()
    x, x_bs = planes(x, "select_positive")
    value = torch.empty(1, dtype=torch.float32, device=x.device)
    count = torch.empty(1, dtype=torch.int64, device=x.device)
    ws = torch.empty(_lib.SELECT_WORKSPACE_BYTES, dtype=torch.uint8, device=x.device)
    check(L.cwfa_select_positive_f32(_p(x), x.shape[0], x[0].numel(), x_bs, int(k), _p(value), _p(count), _p(ws), _stream()),
          "select_positive")
    return value, count


# ------------------------------------------------------------------------------------------------ data preparation
def _f32(v):
    """A number or one-element tensor as the Python float of its fp32 rounding (how torch's scalar operands enter fp32 kernels)."""
    return float(torch.as_tensor(v, dtype=torch.float32).reshape(()).cpu())


def _flat(x, name):
    _dev(x, name)
    return x if x.is_contiguous() else x.contiguous()


def prep_volumes(x, size, offsets, mode="none", t0=0.0, t1=0.0, out_dtype=torch.float32):
    """The crop x[:, :, oh:oh+H, ow:ow+W] of an fp16 [N,D,H0,W0] tensor with the threshold step of ``load_process_volume`` fused in
    (cwfa_prep_volumes_f16; ``mode`` one of none / two / le / maxnorm).  Returns (out, max): max is the one-element device tensor
    of the cropped region's maximum for ``maxnorm``, else None.  ``mode="max_only"`` returns (None, max)."""
    L = _lib.lib()
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("prep_volumes: cwfa_amd runs on MI355X only -- expected a HIP tensor (no CPU fallback exists)")
    if x.dtype != torch.float16 or x.dim() != 4:
        raise TypeError(f"prep_volumes: expected a float16 [N,D,H0,W0] tensor, got {x.dtype} {tuple(x.shape)}")
    if out_dtype not in (torch.float32, torch.float16):
        raise TypeError("prep_volumes: out_dtype must be float32 or float16")
    x = x if x.is_contiguous() else x.contiguous()
    N, D, H0, W0 = x.shape
    (H, W), (oh, ow) = size, offsets
    need_max = mode in ("maxnorm", "max_only")
    mb = torch.empty(2, dtype=torch.float32, device=x.device) if need_max else None
    out = None if mode == "max_only" else torch.empty(N, D, H, W, dtype=out_dtype, device=x.device)
    check(L.cwfa_prep_volumes_f16(_p(x), _p(out), _p(mb), N, D, H0, W0, int(H), int(W), int(oh), int(ow), _lib.PREP_VOL[mode], float(t0),
                                  float(t1), int(out_dtype == torch.float16), _stream()), "prep_volumes")
    return out, (mb[1:2] if need_max else None)


def prep_frames(raw, size, offsets):
    """Raw fp32 frames [N,h,w] -> [N,S0,S1]: NaN -> 0, clip to [0, 50000], fp16 round trip, out[n,r,c] = raw[n, r+oy, c+ox] (0 outside)."""
    L = _lib.lib()
    raw = _flat(raw, "raw")
    if raw.dim() != 3:
        raise ValueError(f"prep_frames: expected [N,h,w], got {tuple(raw.shape)}")
    N, h, w = raw.shape
    out = torch.empty(N, int(size[0]), int(size[1]), dtype=torch.float32, device=raw.device)
    check(L.cwfa_prep_frames_f32(_p(raw), _p(out), N, h, w, int(size[0]), int(size[1]), int(offsets[0]), int(offsets[1]), _stream()), "prep_frames")
    return out


def histogram_range(lo, hi):
    """The outer edges torch.histogram takes for data spanning [lo, hi] (fp32): an empty range is widened by 0.5 on both sides."""
    lo, hi = torch.as_tensor(lo, dtype=torch.float32).reshape(()).cpu(), torch.as_tensor(hi, dtype=torch.float32).reshape(()).cpu()
    if not (torch.isfinite(lo) and torch.isfinite(hi)):
        raise ValueError(f"histogram: the extrema [{float(lo)}, {float(hi)}] are not finite")
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return lo, hi


def histogram(x, bins=10000, range=None, counts=None):
    """(counts int64 [bins] on the device, edges float32 [bins+1] on the CPU) of an fp32 tensor of any shape: torch.histogram's counts
    on the CPU, exactly.  ``range`` = (lo, hi) defaults to the tensor's extrema (one extrema pass); ``counts``: add into these
    (a dataset fed in chunks passes the whole dataset's ``range`` and the running ``counts``)."""
    L = _lib.lib()
    x = _flat(x, "x")
    bins = int(bins)
    if bins < 1 or bins > _lib.PREP_MAX_BINS:
        raise ValueError(f"histogram: bins = {bins} is not in 1 .. {_lib.PREP_MAX_BINS}")
    if range is None:
        if x.numel() == 0:
            raise ValueError("histogram: an empty tensor has no extrema; pass range=(lo, hi)")
        ext = volume_extrema(x.reshape(1, 1, 1, -1))[0, :2].cpu()
        range = (ext[0], ext[1])
    lo, hi = histogram_range(*range)
    if not lo < hi:
        raise ValueError(f"histogram: max {float(hi)} is below min {float(lo)}")
    edges = torch.linspace(lo, hi, bins + 1, dtype=torch.float32)           # host, 10001 floats: bit-equal to torch.histogram's
    if counts is None:
        acc, counts = 0, torch.empty(bins, dtype=torch.int64, device=x.device)
    else:
        acc = 1
        if counts.dtype != torch.int64 or not counts.is_cuda or counts.numel() != bins or not counts.is_contiguous():
            raise ValueError("histogram: counts must be a contiguous int64 [bins] device tensor")
    check(L.cwfa_histogram_f32(_p(x), x.numel(), float(lo), float(hi), _p(edges.to(x.device)), bins, _p(counts), acc, _stream()), "histogram")
    return counts, edges


def prep_apply(x, mode, a=0.0, b=0.0, upper=True, lower=True):
    """In place on a contiguous fp32 tensor: "clamp_zero": x > a -> a (``upper``), then x < b -> 0 (``lower``); "sub_div": (x - a) / b;
    "div_mul": x / a * b.  a and b are rounded to fp32 first.  Returns x."""
    L = _lib.lib()
    _dev(x, "x")
    if not x.is_contiguous():
        raise ValueError("prep_apply: works in place on a contiguous tensor")
    check(L.cwfa_prep_apply_f32(_p(x), x.numel(), _lib.PREP_APPLY[mode], _f32(a), _f32(b), int(bool(upper)) | 2 * int(bool(lower)), _stream()),
          "prep_apply")
    return x


def moments(x, shift=0.0, out=None):
    """float64 [3] on the device: (sum (x - shift), sum (x - shift)^2, count).  ``out``: add to these three (chunked datasets)."""
    L = _lib.lib()
    x = _flat(x, "x")
    shift = float(shift)
    if shift != shift or shift in (float("inf"), float("-inf")):
        raise ValueError(f"moments: the shift {shift} is not finite")
    acc = 1
    if out is None:
        acc, out = 0, torch.empty(3, dtype=torch.float64, device=x.device)
    elif out.dtype != torch.float64 or not out.is_cuda or out.numel() != 3 or not out.is_contiguous():
        raise ValueError("moments: out must be a contiguous float64 [3] device tensor")
    ws = torch.empty(_lib.PREP_MOMENTS_WORKSPACE, dtype=torch.float64, device=x.device)
    check(L.cwfa_moments_f64(_p(x), x.numel(), shift, _p(out), _p(ws), acc, _stream()), "moments")
    return out


def mean_std(tensors):
    """(mean, unbiased std, count) as Python floats (float64) over ALL elements of the given fp32 device tensors, without
    concatenating them: one ``moments`` pass per tensor for the mean, one centred on that mean for the spread (a large mean with a
    small spread survives)."""
    tensors = list(tensors)
    first = None
    for t in tensors:
        first = moments(t, 0.0, first)
    s1, _, n = first.tolist()
    if n == 0:
        return float("nan"), float("nan"), 0
    c = s1 / n
    if c != c or c in (float("inf"), float("-inf")):
        raise ValueError("moments: the data are not finite")
    second = None
    for t in tensors:
        second = moments(t, c, second)
    d1, d2, n = second.tolist()
    var = (d2 - d1 * d1 / n) / (n - 1) if n > 1 else float("nan")
    return c + d1 / n, max(var, 0.0) ** 0.5 if var == var else var, int(n)


def stack_mean_std(x):
    """(mean, std) float32 [D,H,W] over the N samples of [N,D,H,W]: float64 sums centred on the first sample, unbiased std
    (N = 1: NaN, as torch)."""
    L = _lib.lib()
    x = _flat(x, "x")
    if x.dim() < 1 or x.shape[0] < 1:
        raise ValueError("stack_mean_std: needs at least one sample")
    N, m = x.shape[0], x[0].numel()
    mean = torch.empty(x.shape[1:], dtype=torch.float32, device=x.device)
    std = torch.empty_like(mean)
    check(L.cwfa_stack_mean_std_f32(_p(x), _p(mean), _p(std), N, m, m, _stream()), "stack_mean_std")
    return mean, std


# ------------------------------------------------------------------------------------------------ optimiser
def _scalar_arg(t, name, device):
    """A GradScaler scalar (``grad_scale`` / ``found_inf``) as a one-element fp32 tensor on ``device``, without a host round trip."""
    if t is None:
        return None
    if not torch.is_tensor(t) or t.numel() != 1 or t.dtype != torch.float32:
        raise TypeError(f"lion_step: {name} must be a one-element float32 tensor")
    if not t.is_cuda:
        raise RuntimeError(f"lion_step: {name} must live on the HIP device (it is read by the kernel; no CPU fallback exists)")
    return t if t.device == device else t.to(device, non_blocking=True)


def lion_step(params, grads, moments, lr, betas, weight_decay, grad_scale=None, found_inf=None):
    """The Lion update of DESIGN.md section 14 on lists of fp32 device tensors, in place on ``params`` and ``moments``
    (cwfa_lion_step_f32): one launch per ``_lib.LION_MAX_TENSORS`` tensors, the tables passed as kernel arguments.  ``grad_scale`` /
    ``found_inf``: optional one-element fp32 DEVICE tensors (a GradScaler's); the gradients are divided by the first and nothing is
    written when the second is non-zero -- both are read by the kernel, nothing here waits for the device."""
    import struct
    L = _lib.lib()
    params, grads, moments = list(params), list(grads), list(moments)
    if not (len(params) == len(grads) == len(moments)):
        raise ValueError("lion_step: params, grads and moments differ in length")
    if not params:
        return
    flat = []
    for k, (p, g, m) in enumerate(zip(params, grads, moments)):
        _dev(p, f"params[{k}]"), _dev(g, f"grads[{k}]"), _dev(m, f"moments[{k}]")
        if not (p.is_contiguous() and g.is_contiguous() and m.is_contiguous()):
            raise ValueError(f"lion_step: params[{k}], its gradient and its moment must be contiguous (the update is in place)")
        if not (p.numel() == g.numel() == m.numel()):
            raise ValueError(f"lion_step: params[{k}], its gradient and its moment differ in size")
        if not (p.device == g.device == m.device == params[0].device):
            raise ValueError("lion_step: all tensors of one call must live on one device")
        flat += (p.data_ptr(), g.data_ptr(), m.data_ptr(), p.numel())
    dev = params[0].device
    gs, fi = _scalar_arg(grad_scale, "grad_scale", dev), _scalar_arg(found_inf, "found_inf", dev)
    b1, b2 = betas
    size, M = C.sizeof(_lib.LionTable), _lib.LION_MAX_TENSORS
    with torch.cuda.device(dev):
        stream = _stream()
        for i in range(0, len(params), M):
            chunk = flat[4 * i:4 * (i + M)]
            tab = _lib.LionTable.from_buffer_copy(struct.pack(f"=i4x{len(chunk)}q", len(chunk) // 4, *chunk).ljust(size, b"\0"))
            check(L.cwfa_lion_step_f32(C.byref(tab), float(lr), float(b1), float(b2), float(weight_decay), _p(gs), _p(fi), stream),
                  "lion_step")


# ------------------------------------------------------------------------------------------------ training loss
def global_extrema(a, b=None):
    """float32 [EXTREMA_STRIDE] row of ``volume_extrema`` over ALL elements of the contiguous tensor ``a`` (and ``b``) as one sample:
    slots 0, 1 (4, 5) are the global minimum and maximum of a (b).  Exact; an empty tensor gives zeros."""
    L = _lib.lib()
    n = a.numel()
    out = torch.zeros(_lib.EXTREMA_STRIDE, dtype=torch.float32, device=a.device)
    if n:
        ws = torch.empty(L.cwfa_eval_splits(1, n) * 10, dtype=torch.float32, device=a.device)
        check(L.cwfa_volume_extrema_f32(_p(a), _p(b), _p(out), _p(ws), 1, n, n, n, None, _stream()), "global_extrema")
    return out


def wmse_loss(output, target, ths_perc=0.05, gscale=1.0, want_grad=True, extrema=None):
    """The sums of the weighted-MSE loss `wL2` (cwfa_wmse_loss_f32) over two contiguous fp32 device tensors of
    one shape: returns (out, grad) with out float64[2] = (sum (o - t)^2 inside both masks, number of elements inside both masks) and
    grad = d(gscale * out[0]) / d output, exactly zero outside the masks (None unless ``want_grad``; the target's gradient is its
    negative).  The masks are (v - min v) > (max v - min v) * ths_perc in fp32.  ``extrema``: the ``global_extrema(output, target)``
    row if the caller has it already (or has reduced it over its ranks: training.allreduce_extrema); None: computed here.  Two
    launches (three kernels), nothing waits for the device."""
    L = _lib.lib()
    _dev(output, "output"), _dev(target, "target")
    if tuple(output.shape) != tuple(target.shape):
        raise ValueError(f"wmse_loss: output and target differ in shape: {tuple(output.shape)} vs {tuple(target.shape)}")
    if output.device != target.device:
        raise ValueError("wmse_loss: output and target live on different devices")
    if not (output.is_contiguous() and target.is_contiguous()):
        raise ValueError("wmse_loss: output and target must be contiguous")
    n = output.numel()
    with torch.cuda.device(output.device):
        if extrema is None:
            extrema = global_extrema(output, target)
        else:
            _dev(extrema, "extrema")
            if extrema.numel() < _lib.EXTREMA_STRIDE or not extrema.is_contiguous() or extrema.device != output.device:
                raise ValueError(f"wmse_loss: extrema must be a contiguous row of {_lib.EXTREMA_STRIDE} floats on the tensors' device")
        out = torch.empty(2, dtype=torch.float64, device=output.device)
        grad = torch.empty_like(output) if want_grad else None
        ws = torch.empty(max(1, L.cwfa_wmse_workspace_bytes(n) // 8), dtype=torch.float64, device=output.device)
        check(L.cwfa_wmse_loss_f32(_p(output), _p(target), _p(extrema), float(ths_perc), float(gscale), _p(grad), _p(out), _p(ws), n,
                                   _stream()), "wmse_loss")
    return out, grad


# ------------------------------------------------------------------------------------------------ Richardson-Lucy deconvolution
def _cdev(t, name):
    """A contiguous complex64 tensor on the HIP device (the kernels read it as interleaved floats)."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: cwfa_amd runs on MI355X only -- got a {t.device} tensor (no CPU fallback exists)")
    if t.dtype != torch.complex64:
        raise TypeError(f"{name}: expected complex64, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _fdev(t, name):
    _dev(t, name)
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def select_nonzero(x, k=-1, out=None, workspace=None):
    """(value float32[1], count int64[1]) on the device: the k-th smallest of the elements != 0 of the contiguous tensor x (both
    zeros excluded, either sign), k = -1: their lower median -- torch's ``x[x != 0].median()``.  Exact; NaN if k >= count.  ``out``:
    a (value, count) pair and ``workspace``: SELECT_WORKSPACE_BYTES device bytes to write into instead of allocating."""
    L = _lib.lib()
    _fdev(x, "select_nonzero")
    value, count = out if out is not None else (torch.empty(1, dtype=torch.float32, device=x.device),
                                                torch.empty(1, dtype=torch.int64, device=x.device))
    ws = workspace if workspace is not None else torch.empty(_lib.SELECT_WORKSPACE_BYTES, dtype=torch.uint8, device=x.device)
    n = x.numel()
    if n == 0:
        value.fill_(float("nan")), count.zero_()
        return value, count
    check(L.cwfa_select_nonzero_f32(_p(x), 1, n, n, int(k), _p(value), _p(count), _p(ws), _stream()), "select_nonzero")
    return value, count


def deconv_spectrum_mul(a, otf, conj=False, out=None):
    """out[z] = a[z or 0] * otf[z] (``conj``: * conj(otf[z])) on contiguous complex64 tensors whose last two axes are a plane:
    otf holds D planes, a holds D planes or one (broadcast).  ``out`` defaults to a new tensor of otf's shape; ``out=a`` works in
    place when a holds D planes.  otf is never written."""
    L = _lib.lib()
    _cdev(a, "a"), _cdev(otf, "otf")
    if otf.dim() < 2 or a.dim() < 2 or tuple(a.shape[-2:]) != tuple(otf.shape[-2:]):
        raise ValueError(f"deconv_spectrum_mul: planes differ: {tuple(a.shape)} vs {tuple(otf.shape)}")
    n = otf.shape[-2] * otf.shape[-1]
    D, a_planes = (otf.numel() // n, a.numel() // n) if n else (0, 0)
    if out is None:
        out = torch.empty_like(otf)
    _cdev(out, "out")
    if out.numel() != otf.numel():
        raise ValueError("deconv_spectrum_mul: out must have otf's size")
    check(L.cwfa_deconv_spectrum_mul_c64(_p(a), _p(otf), _p(out), D, n, a_planes, int(bool(conj)), _stream()), "deconv_spectrum_mul")
    return out


def deconv_project(p, out=None, window=None, pre=None, post=None, accumulate=False):
    """out[s, 0] (+)= post(sum_z pre(shift(p)[s, z])) over the window (oy, ox, Ho, Wo) of the plane (default: all of it), where
    shift is the reference's ``batch_fftshift2d_real`` (source index = target index + ceil(size / 2)).  p: contiguous [N, D, H, W];
    ``pre``: None / "relu"; ``post``: None / "abs".  Returns out [N, 1, Ho, Wo]."""
    L = _lib.lib()
    _fdev(p, "p")
    if p.dim() != 4:
        raise ValueError(f"deconv_project: expected [N,D,H,W], got {tuple(p.shape)}")
    N, D, H, W = p.shape
    oy, ox, Ho, Wo = (0, 0, H, W) if window is None else (int(v) for v in window)
    if out is None:
        if accumulate:
            raise ValueError("deconv_project: accumulate needs the tensor to add to")
        out = torch.empty(N, 1, Ho, Wo, dtype=torch.float32, device=p.device)
    _fdev(out, "out")
    if out.numel() != N * Ho * Wo:
        raise ValueError(f"deconv_project: out {tuple(out.shape)} does not hold {N} windows of {Ho} x {Wo}")
    check(L.cwfa_deconv_project_f32(_p(p), _p(out), N, D, H, W, Ho, Wo, oy, ox, _lib.DECONV_PRE[pre], _lib.DECONV_POST[post],
                                    int(bool(accumulate)), _stream()), "deconv_project")
    return out


def deconv_ratio(img, est, out, flag):
    """out = img / (est + 1e-8) on contiguous tensors of one size; the int32 device scalar ``flag`` is set to 1 (never cleared) when an
    element of out is NaN or one of img is not finite."""
    L = _lib.lib()
    _fdev(img, "img"), _fdev(est, "est"), _fdev(out, "out")
    if not (img.numel() == est.numel() == out.numel()):
        raise ValueError("deconv_ratio: the tensors differ in size")
    if not flag.is_cuda or flag.dtype != torch.int32 or flag.numel() != 1:
        raise ValueError("deconv_ratio: flag must be a one-element int32 tensor on the HIP device")
    check(L.cwfa_deconv_ratio_f32(_p(img), _p(est), _p(out), _p(flag), img.numel(), _stream()), "deconv_ratio")
    return out


def deconv_clamp(x, median, count, mult):
    """In place clamp(x, 0, median * mult) with ``median`` (float32[1]) and ``count`` (int64[1]) on the device, as ``select_nonzero``
    returns them; nothing happens when count is 0."""
    L = _lib.lib()
    _fdev(x, "x"), _dev(median, "median")
    if not count.is_cuda or count.dtype != torch.int64 or count.numel() != 1 or median.numel() != 1:
        raise ValueError("deconv_clamp: median / count must be one-element float32 / int64 tensors on the HIP device")
    check(L.cwfa_deconv_clamp_f32(_p(x), x.numel(), _p(median), _p(count), float(mult), _stream()), "deconv_clamp")
    return x


def deconv_update(obj_pad, b, obj, po):
    """obj_pad[..., po:po+obj, po:po+obj] *= shift(b)[..., po:po+obj, po:po+obj] in place on contiguous [.., D, F, F] tensors of one
    shape (shift as in ``deconv_project``); nothing outside the window is read or written."""
    L = _lib.lib()
    _fdev(obj_pad, "obj_pad"), _fdev(b, "b")
    if obj_pad.dim() < 2 or tuple(obj_pad.shape) != tuple(b.shape) or obj_pad.shape[-1] != obj_pad.shape[-2]:
        raise ValueError(f"deconv_update: expected two [.., F, F] tensors of one shape, got {tuple(obj_pad.shape)} and {tuple(b.shape)}")
    F = obj_pad.shape[-1]
    D = obj_pad.numel() // (F * F) if F else 0
    check(L.cwfa_deconv_update_f32(_p(obj_pad), _p(b), D, F, int(obj), int(po), _stream()), "deconv_update")
    return obj_pad


def deconv_accel_slab(D, obj, device):
    """The zeroed float64 slab [rows, 2] ``deconv_update_accel`` adds its block partials to, for chunks of at most D depths of an
    obj x obj window; ``deconv_alpha`` leaves it zeroed again."""
    rows = int(D) * ((int(obj) * int(obj) + _lib.DECONV_ACCEL_UNITS - 1) // _lib.DECONV_ACCEL_UNITS)
    return torch.zeros(max(rows, 1), 2, dtype=torch.float64, device=device)


def _slab(slab, name):
    if not torch.is_tensor(slab) or not slab.is_cuda or slab.dtype != torch.float64 or not slab.is_contiguous() or slab.numel() % 2:
        raise ValueError(f"{name}: slab must be a contiguous float64 tensor [rows, 2] on the HIP device (deconv_accel_slab)")
    return slab


def _scalar(t, dtype, name, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or t.numel() != 1:
        raise ValueError(f"{name}: {what} must be a one-element {str(dtype)[6:]} tensor on the HIP device")
    return t


def _window(obj_pad, wins, obj, name):
    """(D, F) of a contiguous padded tensor [.., D, F, F] and window tensors [.., D, obj, obj] of as many depths."""
    _fdev(obj_pad, "obj_pad")
    if obj_pad.dim() < 2 or obj_pad.shape[-1] != obj_pad.shape[-2]:
        raise ValueError(f"{name}: expected a padded tensor [.., F, F], got {tuple(obj_pad.shape)}")
    F, obj = obj_pad.shape[-1], int(obj)
    D = obj_pad.numel() // (F * F) if F else 0
    for w_name, w in wins:
        _fdev(w, w_name)
        if w.dim() < 2 or tuple(w.shape[-2:]) != (obj, obj) or w.numel() != D * obj * obj:
            raise ValueError(f"{name}: {w_name} {tuple(w.shape)} does not hold {D} windows of {obj} x {obj}")
    return D, F


def deconv_update_accel(obj_pad, b, g, x_new, slab, obj, po):
    """The accelerated form of ``deconv_update`` for one depth chunk: x_new = window(obj_pad) * window(shift(b)), the same fp32
    product; the step x_new - window(obj_pad) replaces the previous step in ``g`` (in place), and the float64 partials of
    sum(step * previous step) and sum(previous step^2) are added to ``slab``.  obj_pad and b [.., D, F, F] are only read; g and
    x_new are contiguous [.., D, obj, obj]."""
    L = _lib.lib()
    _fdev(b, "b")
    D, F = _window(obj_pad, (("g", g), ("x_new", x_new)), obj, "deconv_update_accel")
    if tuple(obj_pad.shape) != tuple(b.shape):
        raise ValueError(f"deconv_update_accel: expected two [.., F, F] tensors of one shape, got {tuple(obj_pad.shape)} and {tuple(b.shape)}")
    _slab(slab, "deconv_update_accel")
    check(L.cwfa_deconv_update_accel_f32(_p(obj_pad), _p(b), _p(g), _p(x_new), _p(g), _p(slab), slab.numel() // 2, D, F, int(obj), int(po),
                                         _stream()), "deconv_update_accel")
    return x_new


def deconv_alpha(slab, alpha_max, alpha):
    """alpha (float32[1] on the device) = clamp(sum(slab[:, 0]) / sum(slab[:, 1]), 0, alpha_max), 0 where that quotient is not
    finite; the slab is zeroed.  Nothing comes back to the host."""
    L = _lib.lib()
    _slab(slab, "deconv_alpha"), _scalar(alpha, torch.float32, "deconv_alpha", "alpha")
    check(L.cwfa_deconv_alpha_f64(_p(slab), slab.numel() // 2, float(alpha_max), _p(alpha), _stream()), "deconv_alpha")
    return alpha


def deconv_predict(obj_pad, x_new, x_prev, alpha, obj, po):
    """obj_pad[..., po:po+obj, po:po+obj] = max(x_new + alpha * (x_new - x_prev), 0) with ``alpha`` a float32[1] on the device and
    three separately rounded fp32 operations; nothing outside the window is written."""
    L = _lib.lib()
    D, F = _window(obj_pad, (("x_new", x_new), ("x_prev", x_prev)), obj, "deconv_predict")
    _scalar(alpha, torch.float32, "deconv_predict", "alpha")
    check(L.cwfa_deconv_predict_f32(_p(obj_pad), _p(x_new), _p(x_prev), _p(alpha), D, F, int(obj), int(po), _stream()), "deconv_predict")
    return obj_pad


def deconv_penalty_slab(D, obj, device):
    """The zeroed float64 slab [rows] ``deconv_update_map`` and ``deconv_update_accel_map`` add the block partials of the prior's
    penalty to, for chunks of at most D depths of an obj x obj window; ``deconv_penalty`` leaves it zeroed again."""
    # sized for the plain kernel's element-by-element walk, the most rows either kernel can use: a launch picks its 16-byte path
    # from the pointers' alignment, and that path and the accelerated walk (1024 units per block) fill only the front of the slab
    rows = int(D) * ((int(obj) * int(obj) + _lib.DECONV_UPDATE_UNITS - 1) // _lib.DECONV_UPDATE_UNITS)
    return torch.zeros(max(rows, 1), dtype=torch.float64, device=device)


def _pen_slab(slab, name):
    if slab is None:
        return None, 0
    if not torch.is_tensor(slab) or not slab.is_cuda or slab.dtype != torch.float64 or not slab.is_contiguous():
        raise ValueError(f"{name}: penalty_slab must be a contiguous float64 tensor on the HIP device (deconv_penalty_slab)")
    return _p(slab), slab.numel()


def _trace(trace, index, name):
    if not torch.is_tensor(trace) or not trace.is_cuda or trace.dtype != torch.float64 or not trace.is_contiguous():
        raise ValueError(f"{name}: trace must be a contiguous float64 tensor on the HIP device")
    if not 0 <= int(index) < trace.numel():
        raise ValueError(f"{name}: element {index} is not inside a trace of {trace.numel()}")
    return trace


def deconv_update_map(obj_pad, b, mu, w, obj, po, penalty_slab=None):
    """``deconv_update`` under a Gaussian prior N(mu, 1 / w) per voxel, for one depth chunk, in place: the window of obj_pad becomes
    M(window * window(shift(b)), mu, w), the positive root of w x^2 + (1 - w mu) x - a = 0 in its cancellation-free fp32 form
    (DESIGN.md section 21); w = 0 gives ``deconv_update``'s bits.  mu and w are contiguous [.., D, obj, obj] and only read.  With
    ``penalty_slab`` (``deconv_penalty_slab``) the float64 partials of sum(0.5 w (window - mu)^2) of the window as read are added
    to it."""
    L = _lib.lib()
    _fdev(b, "b")
    D, F = _window(obj_pad, (("mu", mu), ("w", w)), obj, "deconv_update_map")
    if tuple(obj_pad.shape) != tuple(b.shape):
        raise ValueError(f"deconv_update_map: expected two [.., F, F] tensors of one shape, got {tuple(obj_pad.shape)} and {tuple(b.shape)}")
    pen, pen_rows = _pen_slab(penalty_slab, "deconv_update_map")
    check(L.cwfa_deconv_update_map_f32(_p(obj_pad), _p(b), _p(mu), _p(w), pen, pen_rows, D, F, int(obj), int(po), _stream()),
          "deconv_update_map")
    return obj_pad


def deconv_update_accel_map(obj_pad, b, g, x_new, mu, w, slab, obj, po, penalty_slab=None):
    """``deconv_update_accel`` under the prior of ``deconv_update_map``: x_new = M(window(obj_pad) * window(shift(b)), mu, w), the
    step x_new - window(obj_pad) replaces the previous step in ``g``, ``slab`` receives the same two sums; ``penalty_slab`` as in
    ``deconv_update_map`` (the penalty of window(obj_pad))."""
    L = _lib.lib()
    _fdev(b, "b")
    D, F = _window(obj_pad, (("g", g), ("x_new", x_new), ("mu", mu), ("w", w)), obj, "deconv_update_accel_map")
    if tuple(obj_pad.shape) != tuple(b.shape):
        raise ValueError(f"deconv_update_accel_map: expected two [.., F, F] tensors of one shape, got {tuple(obj_pad.shape)} and "
                         f"{tuple(b.shape)}")
    _slab(slab, "deconv_update_accel_map")
    pen, pen_rows = _pen_slab(penalty_slab, "deconv_update_accel_map")
    check(L.cwfa_deconv_update_accel_map_f32(_p(obj_pad), _p(b), _p(g), _p(mu), _p(w), _p(x_new), _p(g), _p(slab), slab.numel() // 2, pen,
                                             pen_rows, D, F, int(obj), int(po), _stream()), "deconv_update_accel_map")
    return x_new


def deconv_penalty(penalty_slab, trace, index):
    """trace[index] += the sum of ``penalty_slab`` in one fixed order (on top of the likelihood ``deconv_poisson_nll`` wrote there);
    the slab is zeroed.  Nothing comes back to the host."""
    L = _lib.lib()
    if penalty_slab is None:
        raise ValueError("deconv_penalty: penalty_slab must be a contiguous float64 tensor on the HIP device (deconv_penalty_slab)")
    pen, pen_rows = _pen_slab(penalty_slab, "deconv_penalty")
    _trace(trace, index, "deconv_penalty")
    check(L.cwfa_deconv_penalty_f64(pen, pen_rows, _p(trace), int(index), trace.numel(), _stream()), "deconv_penalty")
    return trace


def deconv_poisson_nll(img, est, trace, index, workspace=None):
    """trace[index] = sum(est - img * log(est + 1e-8)) in float64 over two contiguous float32 tensors of one size; ``trace`` a
    contiguous float64 vector on the device, ``workspace`` DECONV_NLL_WORKSPACE_BYTES device bytes to use instead of allocating."""
    L = _lib.lib()
    _fdev(img, "img"), _fdev(est, "est")
    if img.numel() != est.numel():
        raise ValueError("deconv_poisson_nll: the tensors differ in size")
    if not torch.is_tensor(trace) or not trace.is_cuda or trace.dtype != torch.float64 or not trace.is_contiguous():
        raise ValueError("deconv_poisson_nll: trace must be a contiguous float64 tensor on the HIP device")
    if not 0 <= int(index) < trace.numel():
        raise ValueError(f"deconv_poisson_nll: element {index} is not inside a trace of {trace.numel()}")
    ws = workspace if workspace is not None else torch.empty(_lib.DECONV_NLL_WORKSPACE_BYTES, dtype=torch.uint8, device=img.device)
    if not ws.is_cuda or ws.numel() * ws.element_size() < _lib.DECONV_NLL_WORKSPACE_BYTES:
        raise ValueError(f"deconv_poisson_nll: the workspace needs {_lib.DECONV_NLL_WORKSPACE_BYTES} device bytes")
    check(L.cwfa_deconv_poisson_nll_f32(_p(img), _p(est), img.numel(), _p(trace), int(index), trace.numel(), _p(ws), _stream()),
          "deconv_poisson_nll")
    return trace


# ------------------------------------------------------------------------------------------------ neuron detection
def activity_state(shape, device):
    """The per-voxel state of a streaming activity map for volumes of ``shape``: (x0 fp32, s1 float64, s2 float64, vmax fp32,
    vmin fp32), 28 bytes per voxel, uninitialised -- the first ``activity_update`` (``first=True``) writes all of it."""
    f = lambda dt: torch.empty(tuple(shape), dtype=dt, device=device)
    return f(torch.float32), f(torch.float64), f(torch.float64), f(torch.float32), f(torch.float32)


def _activity(state, what):
    if len(state) != 5:
        raise ValueError(f"{what}: the state is (x0, s1, s2, vmax, vmin)")
    for t, dt in zip(state, (torch.float32, torch.float64, torch.float64, torch.float32, torch.float32)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.shape != state[0].shape:
            raise ValueError(f"{what}: the state is five contiguous tensors of one shape on the HIP device (ops.activity_state)")
    return state[0].numel()


def activity_update(x, state, first):
    """Add the chunk ``x`` [T', ...] (float32; contiguous volumes, any time stride of at least a volume) to ``state``
    (``activity_state``).  ``first``: the state is initialised from x[0].  Per voxel the additions are those of ``stack_mean_std`` in
    its order, however the series is chunked."""
    L = _lib.lib()
    _dev(x, "x")
    m = _activity(state, "activity_update")
    if x.dim() < 1 or tuple(x.shape[1:]) != tuple(state[0].shape):
        raise ValueError(f"activity_update: a chunk [T', {', '.join(str(s) for s in state[0].shape)}] is expected, got {tuple(x.shape)}")
    T = x.shape[0]
    if first and T < 1:
        raise ValueError("activity_update: the first chunk needs at least one volume")
    if T and m and (not x[0].is_contiguous() or (T > 1 and x.stride(0) < m)):
        x = x.contiguous()
    ss = x.stride(0) if T > 1 else m
    check(L.cwfa_activity_update_f32(_p(x), *(_p(t) for t in state), T, m, ss, int(bool(first)), _stream()), "activity_update")
    return state


def activity_finish(state, count, kind="std"):
    """(score, mean, std) float32 maps from ``state`` after ``count`` samples: mean and std are the bits of ``stack_mean_std`` on the
    whole series (unbiased, NaN for one sample); ``kind``: "std", "range" (vmax - vmin), "peak" (vmax - mean) or "snr"
    ((vmax - mean) / std, 0 where std == 0), in separately rounded fp32 operations."""
    L = _lib.lib()
    if kind not in _lib.ACTIVITY_KIND:
        raise ValueError(f"activity_finish: kind is one of {sorted(_lib.ACTIVITY_KIND)}, got {kind!r}")
    m = _activity(state, "activity_finish")
    if int(count) < 1:
        raise ValueError("activity_finish: needs at least one sample")
    score, mean, std = (torch.empty_like(state[0]) for _ in range(3))
    check(L.cwfa_activity_finish_f32(*(_p(t) for t in state), int(count), _lib.ACTIVITY_KIND[kind], _p(mean), _p(std), _p(score), m,
                                     _stream()), "activity_finish")
    return score, mean, std


def _corr(state, cc, neighbours, what):
    if neighbours not in _lib.CORR_FORWARD:
        raise ValueError(f"{what}: neighbours is one of {sorted(_lib.CORR_FORWARD)}, got {neighbours!r}")
    m = _activity(state, what)
    if state[0].dim() != 3:
        raise ValueError(f"{what}: the state of [D,H,W] volumes is expected, got {tuple(state[0].shape)}")
    if (not torch.is_tensor(cc) or not cc.is_cuda or cc.dtype != torch.float64 or not cc.is_contiguous()
            or tuple(cc.shape) != (_lib.CORR_FORWARD[neighbours], *state[0].shape)):
        raise ValueError(f"{what}: cc is a contiguous float64 tensor [{_lib.CORR_FORWARD[neighbours]}, D, H, W] on the HIP device "
                         f"(ops.correlation_state)")
    return m


def correlation_state(shape, device, neighbours):
    """The pair sums of a streaming local-correlation map for [D,H,W] volumes of ``shape``: float64 [K,D,H,W], K = 3, 4 or 13 forward
    offsets for ``neighbours`` = 6 (faces), 8 (the in-plane ring) or 26 (the cube); 8 K bytes per voxel beside the 28 of
    ``activity_state``, uninitialised -- the first ``activity_update_corr`` (``first=True``) writes all of it."""
    if neighbours not in _lib.CORR_FORWARD:
        raise ValueError(f"correlation_state: neighbours is one of {sorted(_lib.CORR_FORWARD)}, got {neighbours!r}")
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or min(shape) < 0:
        raise ValueError(f"correlation_state: shape is (D, H, W), got {shape!r}")
    return torch.empty((_lib.CORR_FORWARD[neighbours], *shape), dtype=torch.float64, device=device)


def activity_update_corr(x, state, cc, neighbours, first):
    """``activity_update`` of the chunk ``x`` [T',D,H,W] -- ``state`` comes out bit for bit as that writes it -- which in the same read
    of the chunk adds, per voxel i and forward offset o_k of ``neighbours``, d_i(t) d_j(t) (j = i + o_k, d = x - x0 in float64) to
    ``cc`` (``correlation_state``) in time order; 0.0 where j is outside the volume.  Any chunking gives the same bits."""
    L = _lib.lib()
    _dev(x, "x")
    m = _corr(state, cc, neighbours, "activity_update_corr")
    if x.dim() != 4 or tuple(x.shape[1:]) != tuple(state[0].shape):
        raise ValueError(f"activity_update_corr: a chunk [T', {', '.join(str(s) for s in state[0].shape)}] is expected, "
                         f"got {tuple(x.shape)}")
    T = x.shape[0]
    if first and T < 1:
        raise ValueError("activity_update_corr: the first chunk needs at least one volume")
    if T and m and (not x[0].is_contiguous() or (T > 1 and x.stride(0) < m)):
        x = x.contiguous()
    ss = x.stride(0) if T > 1 else m
    check(L.cwfa_activity_update_corr_f32(_p(x), *(_p(t) for t in state), _p(cc), T, *state[0].shape, ss, int(neighbours), int(bool(first)),
                                          _stream()), "activity_update_corr")
    return state, cc


def correlation_finish(state, cc, count, neighbours):
    """The local-correlation map, float32 [D,H,W], after ``count`` samples: per voxel the mean over its in-volume neighbours of the
    Pearson correlation of the two series, evaluated in float64 from ``state`` and ``cc``; a pair with a constant series, or one
    holding NaN or inf, counts with 0, so the map holds no NaN and lies in [-1, 1] up to rounding.  The state is only read."""
    L = _lib.lib()
    _corr(state, cc, neighbours, "correlation_finish")
    if int(count) < 1:
        raise ValueError("correlation_finish: needs at least one sample")
    score = torch.empty_like(state[0])
    check(L.cwfa_activity_corr_finish_f32(_p(state[1]), _p(state[2]), _p(cc), int(count), *state[0].shape, int(neighbours), _p(score),
                                          _stream()), "correlation_finish")
    return score


# ------------------------------------------------------------------------------------------------ regression maps
RegressionState = namedtuple("RegressionState", ["plain", "p", "sr", "srr", "rows"])
RegressionDesign = namedtuple("RegressionDesign", ["gdiag", "ginv", "status"])


def regression_state(shape, device, k):
    """The state of a streaming regression of [D,H,W] volumes of ``shape`` on ``k`` regressors:
    ``plain`` = ``activity_state`` (28 bytes per voxel), ``p`` float64 [k,D,H,W] (8 k bytes per voxel), and the regressors' own sums
    ``sr`` float64 [k], ``srr`` float64 [k,k] and row count ``rows`` int64 [1], all uninitialised -- the first
    ``activity_update_regress`` / ``regress_rows`` (``first=True``) write all of it."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or min(shape) < 0:
        raise ValueError(f"regression_state: shape is (D, H, W), got {shape!r}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.REGRESS_MAX_K:
        raise ValueError(f"regression_state: 1 .. {_lib.REGRESS_MAX_K} regressors, got {k!r}")
    f = lambda *s: torch.empty(s, dtype=torch.float64, device=device)
    return RegressionState(activity_state(shape, device), f(k, *shape), f(k), f(k, k), torch.empty(1, dtype=torch.int64, device=device))


def _regress(st, what):
    if not isinstance(st, RegressionState):
        raise ValueError(f"{what}: the state is an ops.RegressionState (ops.regression_state)")
    m = _activity(st.plain, what)
    if st.plain[0].dim() != 3:
        raise ValueError(f"{what}: the state of [D,H,W] volumes is expected, got {tuple(st.plain[0].shape)}")
    k = st.p.shape[0] if torch.is_tensor(st.p) and st.p.dim() == 4 else 0
    for t, dt, shape in ((st.p, torch.float64, (k, *st.plain[0].shape)), (st.sr, torch.float64, (k,)), (st.srr, torch.float64, (k, k)),
                         (st.rows, torch.int64, (1,))):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"{what}: p [K,D,H,W], sr [K], srr [K,K] (float64) and rows [1] (int64) are contiguous tensors on the HIP "
                             f"device (ops.regression_state)")
    if not 1 <= k <= _lib.REGRESS_MAX_K:
        raise ValueError(f"{what}: 1 .. {_lib.REGRESS_MAX_K} regressors, got {k}")
    return m, k


def _regress_rows(rows, T, k, what):
    if not torch.is_tensor(rows) or rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[1] != k:
        raise ValueError(f"{what}: rows is a float64 tensor [T', {k}], got "
                         f"{(tuple(rows.shape), rows.dtype) if torch.is_tensor(rows) else type(rows)}")
    if T is not None and rows.shape[0] != T:
        raise ValueError(f"{what}: {rows.shape[0]} rows for {T} volumes")
    if not rows.is_cuda:
        raise RuntimeError(f"{what}: cwfa_amd runs on MI355X only -- got {rows.device} rows (no CPU fallback exists)")
    return rows.contiguous()


def activity_update_regress(x, rows, st, first):
    """``activity_update`` of the chunk ``x`` [T',D,H,W] -- ``st.plain`` comes out bit for bit as that writes it -- which in the same
    read of the chunk adds d(t) r[t,k] (d = x - x0 in float64) to ``st.p[k]`` per voxel, in time order; ``rows``: the chunk's float64
    [T',K] on the device.  Any chunking gives the same bits.  The regressors' own sums are ``regress_rows``'."""
    L = _lib.lib()
    _dev(x, "x")
    m, k = _regress(st, "activity_update_regress")
    if x.dim() != 4 or tuple(x.shape[1:]) != tuple(st.plain[0].shape):
        raise ValueError(f"activity_update_regress: a chunk [T', {', '.join(str(s) for s in st.plain[0].shape)}] is expected, "
                         f"got {tuple(x.shape)}")
    T = x.shape[0]
    rows = _regress_rows(rows, T, k, "activity_update_regress")
    if first and T < 1:
        raise ValueError("activity_update_regress: the first chunk needs at least one volume")
    if T and m and (not x[0].is_contiguous() or (T > 1 and x.stride(0) < m)):
        x = x.contiguous()
    ss = x.stride(0) if T > 1 else m
    check(L.cwfa_activity_update_regress_f32(_p(x), _p(rows), *(_p(t) for t in st.plain), _p(st.p), T, k, m, ss, int(bool(first)),
                                             _stream()), "activity_update_regress")
    return st


def regress_rows(rows, st, first):
    """Add the float64 ``rows`` [T',K] to ``st.sr`` (sums), ``st.srr`` (sums of products) and ``st.rows`` (their number), in time
    order; ``first`` starts them from 0."""
    L = _lib.lib()
    _, k = _regress(st, "regress_rows")
    rows = _regress_rows(rows, None, k, "regress_rows")
    check(L.cwfa_regress_rows_f64(_p(rows), rows.shape[0], k, _p(st.sr), _p(st.srr), _p(st.rows), int(bool(first)), _stream()),
          "regress_rows")
    return st


def regress_design(st, count, rcond=1e-10):
    """``RegressionDesign(gdiag [K], ginv [K,K], status int32 [2])`` on the device from the regressors' sums after ``count`` samples:
    the diagonal of G = Srr - Sr Sr' / N and G's inverse by a Cholesky factorisation in one thread.  ``status[0]`` != 0 (a key of
    ``_lib.REGRESS_STATUS``; ``status[1]``: the regressor) when a pivot is not above ``rcond`` times its diagonal entry, an entry is
    not finite or ``st.rows`` != ``count``.  Nothing is read back: the caller reads the status."""
    L = _lib.lib()
    _, k = _regress(st, "regress_design")
    if int(count) < 1:
        raise ValueError("regress_design: needs at least one sample")
    if not 0.0 <= float(rcond) < 1.0:
        raise ValueError(f"regress_design: rcond is in [0, 1), got {rcond!r}")
    dev = st.sr.device
    des = RegressionDesign(torch.empty(k, dtype=torch.float64, device=dev), torch.empty(k, k, dtype=torch.float64, device=dev),
                           torch.empty(2, dtype=torch.int32, device=dev))
    check(L.cwfa_regress_design_f64(_p(st.sr), _p(st.srr), _p(st.rows), int(count), k, float(rcond), _p(des.gdiag), _p(des.ginv),
                                    _p(des.status), _stream()), "regress_design")
    return des


def regress_want(want, count, k, what):
    """The mask of ``want`` (names out of "corr", "beta", "t", "r2"), refusing an unknown name, an empty set and ``t`` without a
    degree of freedom."""
    names = (want,) if isinstance(want, str) else tuple(want)
    if not names or any(n not in _lib.REGRESS_WANT for n in names):
        raise ValueError(f"{what}: want is a non-empty subset of {tuple(_lib.REGRESS_WANT)}, got {want!r}")
    if "t" in names and int(count) - k - 1 < 1:
        raise ValueError(f"{what}: t needs N - K - 1 >= 1 degrees of freedom, got {int(count)} samples for {k} regressors")
    return sum(_lib.REGRESS_WANT[n] for n in set(names))


def regress_finish(st, design, count, want=("corr", "beta", "t", "r2")):
    """(corr [K,D,H,W], beta [K,D,H,W], t [K,D,H,W], r2 [D,H,W]) float32 from the state after ``count`` samples and ``design``
    (``regress_design``), ``None`` for what ``want`` does not name; the formulae of DESIGN.md section 34.1 in float64.  A voxel whose
    series is constant or holds NaN or inf is 0 in every map.  The state is only read."""
    L = _lib.lib()
    m, k = _regress(st, "regress_finish")
    if int(count) < 1:
        raise ValueError("regress_finish: needs at least one sample")
    mask = regress_want(want, count, k, "regress_finish")
    if (not isinstance(design, RegressionDesign) or any(not torch.is_tensor(t) or not t.is_cuda or not t.is_contiguous() for t in design)
            or tuple(design.gdiag.shape) != (k,) or tuple(design.ginv.shape) != (k, k) or design.gdiag.dtype != torch.float64
            or design.ginv.dtype != torch.float64):
        raise ValueError(f"regress_finish: design is the ops.RegressionDesign of {k} regressors (ops.regress_design)")
    shape = tuple(st.plain[0].shape)
    out = [torch.empty((k, *shape) if n != "r2" else shape, dtype=torch.float32, device=st.p.device) if mask & bit else None
           for n, bit in _lib.REGRESS_WANT.items()]
    check(L.cwfa_regress_finish_f32(_p(st.plain[1]), _p(st.plain[2]), _p(st.p), _p(st.sr), _p(design.gdiag), _p(design.ginv), int(count),
                                    k, m, mask, *(_p(t) for t in out), _stream()), "regress_finish")
    return tuple(out)


def _triple(v, name, what):
    try:
        t = tuple(int(a) for a in v)
    except (TypeError, ValueError):
        t = ()
    if len(t) != 3 or any(a != b for a, b in zip(t, v)):
        raise ValueError(f"{what}: {name} is three integers (z, y, x), got {v!r}")
    return t


def local_maxima_args(dist, margin, n_max, capacity, what):
    """``local_maxima``'s host-side arguments, checked before anything touches the device: (dist, margin, n_max, capacity)."""
    dist, margin = _triple(dist, "dist", what), _triple(margin, "margin", what)
    if any(d < 0 or d > _lib.NMAX_MAX_DIST for d in dist):
        raise ValueError(f"{what}: half-widths {dist} are not in 0 .. {_lib.NMAX_MAX_DIST}")
    if any(v < 0 for v in margin) or int(capacity) < 0 or (n_max is not None and int(n_max) < 0):
        raise ValueError(f"{what}: margin, capacity and n_max are not negative")
    return dist, margin, None if n_max is None else int(n_max), int(capacity)


def peak_order(bits, lin):
    """The order of ``local_maxima``'s result: the 64-bit keys ord(score) << 32 | (0xFFFFFFFF - index) of numpy arrays of fp32 bit
    patterns (uint32) and linear indices, formed from the pair alone; peaks are listed by descending key."""
    import numpy as np
    s = bits.astype(np.uint32).view(np.float32) + np.float32(0.0)
    u = s.view(np.uint32)
    o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    o = np.where(np.isnan(s), np.uint32(0), o)
    return (o.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - lin.astype(np.uint64))


def local_maxima(score, thr, dist, margin=(0, 0, 0), n_max=None, capacity=1 << 20):
    """The 3-D local maxima of a float32 device map [D,H,W]: the voxels that are not NaN, at least ``thr``, at least ``margin``
    (z, y, x) from every face and the maximum of the box of half-widths ``dist`` (z, y, x; 0 .. 16 each) around them under the total
    order "by value, ties to the lower linear index" (a plateau gives one voxel per window).  Returns, on the host,
    (zyx int32 [K,3], scores float32 [K], total): ordered by score descending, then index ascending, the first ``n_max`` of ``total``
    peaks.  ``capacity``: entries of the device buffer of the first run; if there are more peaks the kernels run once more with
    room for all of them -- the candidate set is never truncated."""
    import numpy as np
    dist, margin, n_max, capacity = local_maxima_args(dist, margin, n_max, capacity, "local_maxima")
    L = _lib.lib()
    _dev(score, "score")
    if score.dim() != 3:
        raise ValueError(f"local_maxima: a [D,H,W] map is expected, got {tuple(score.shape)}")
    score = score if score.is_contiguous() else score.contiguous()
    D, H, W = score.shape
    n = score.numel()
    if n > 1 << 32:
        raise ValueError(f"local_maxima: {D} x {H} x {W} voxels do not fit a 32-bit linear index")
    ws = torch.empty(max(n, 1), dtype=torch.int64, device=score.device)
    count = torch.empty(1, dtype=torch.int64, device=score.device)
    cap = min(int(capacity), n)
    while True:
        out = torch.empty(max(cap, 1), 2, dtype=torch.int32, device=score.device)
        check(L.cwfa_local_maxima_f32(_p(score), D, H, W, _f32(thr), *dist, *margin, _p(ws), _p(out), cap, _p(count), _stream()),
              "local_maxima")
        total = int(count.cpu()[0])
        if total <= cap:
            break
        cap = total
    pairs = out[:total].cpu().numpy().view(np.uint32)
    bits, lin = pairs[:, 0], pairs[:, 1].astype(np.int64)
    order = np.argsort(peak_order(bits, lin))[::-1]
    if n_max is not None:
        order = order[:int(n_max)]
    lin = lin[order]
    zyx = np.stack([lin // (H * W), lin // W % H, lin % W], axis=1).astype(np.int32) if len(lin) else np.zeros((0, 3), dtype=np.int32)
    return zyx, bits[order].view(np.float32).copy(), total


# ------------------------------------------------------------------------------------------------ sparse-activity extraction
_STACK_DTYPE = {torch.float32: 0, torch.float16: 1}


def _stack(x, what):
    """A [T, ...] fp32 / fp16 device stack as (tensor, dtype code, T, P, frame stride): frames contiguous, any stride of at least a
    frame between them (a band of rows of every frame qualifies without a copy)."""
    if not torch.is_tensor(x):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(x)}")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: cwfa_amd runs on MI355X only -- got a {x.device} tensor (no CPU fallback exists)")
    if x.dtype not in _STACK_DTYPE:
        raise TypeError(f"{what}: expected a float32 or float16 stack, got {x.dtype}")
    if x.dim() < 2:
        raise ValueError(f"{what}: a stack [T, ...] is expected, got {tuple(x.shape)}")
    T, P = int(x.shape[0]), 1
    for s in x.shape[1:]:
        P *= int(s)
    if T and P and (not x[0].is_contiguous() or (T > 1 and x.stride(0) < P)):
        x = x.contiguous()
    return x, _STACK_DTYPE[x.dtype], T, P, (x.stride(0) if T > 1 and P else P)


def _vec(t, n, name, what, dtype=torch.float32):
    """A contiguous device tensor of ``n`` elements of ``dtype`` (any shape)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{what}: {name} must be a tensor on the HIP device (no CPU fallback exists)")
    if t.dtype != dtype or t.numel() != n:
        raise ValueError(f"{what}: {name} holds {n} {dtype} values, got {tuple(t.shape)} {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def temporal_lds_frames(dtype, transformed=False):
    """The largest T the one-read form of ``temporal_select`` accepts for a stack of ``dtype`` with (``transformed``) or without a
    background (a, b).  Host only."""
    if dtype not in _STACK_DTYPE:
        raise TypeError(f"temporal_lds_frames: float32 or float16, got {dtype}")
    return int(_lib.lib().cwfa_temporal_select_lds_frames(_STACK_DTYPE[dtype], int(bool(transformed))))


def temporal_select(stack, ranks, a=None, b=None, form="auto"):
    """Per-pixel temporal order statistics of a [T, ...] fp32 / fp16 device stack: out[k] (float32, the shape of a frame) holds the
    ``ranks[k]``-th smallest (from 0) of the T values of every pixel, for 1 to 4 ranks; the result is an element of the series, bit
    for bit (-0 and +0 are one value, returned as +0).  With ``a`` [T] and ``b`` (a frame) the series is x - a[t] * b[p], formed on
    load in fp32.  ``form``: "lds" (one read of the stack, T up to ``temporal_lds_frames``), "stream" (any T) or "auto"."""
    L = _lib.lib()
    stack, dt, T, P, fs = _stack(stack, "temporal_select")
    if form not in _lib.SELECT_FORM:
        raise ValueError(f"temporal_select: form is one of {sorted(_lib.SELECT_FORM)}, got {form!r}")
    ranks = [int(r) for r in ranks]
    if not 1 <= len(ranks) <= 4:
        raise ValueError(f"temporal_select: 1 to 4 ranks, got {len(ranks)}")
    if T < 1 or any(r < 0 or r >= T for r in ranks):
        raise ValueError(f"temporal_select: ranks {ranks} are not in 0 .. {T - 1}")
    if (a is None) != (b is None):
        raise ValueError("temporal_select: a and b are given together or not at all")
    if a is not None:
        a, b = _vec(a, T, "a", "temporal_select"), _vec(b, P, "b", "temporal_select")
    out = torch.empty((len(ranks),) + tuple(stack.shape[1:]), dtype=torch.float32, device=stack.device)
    check(L.cwfa_temporal_select(_p(stack), dt, T, P, fs, _p(a), _p(b), (C.c_int * len(ranks))(*ranks), len(ranks), _p(out),
                                 _lib.SELECT_FORM[form], _stream()), "temporal_select")
    return out


def frame_dots(stack, b, sums=None):
    """float64 [T + 1] on the device: sums[t] = sum_p stack[t, p] * b[p] and sums[T] = sum_p b[p]^2, every product formed in float64,
    partial sums added in a fixed order (bitwise repeatable).  ``sums``: add to these (bands of rows of one stack add up)."""
    L = _lib.lib()
    stack, dt, T, P, fs = _stack(stack, "frame_dots")
    b = _vec(b, P, "b", "frame_dots")
    acc = 1
    if sums is None:
        acc, sums = 0, torch.empty(T + 1, dtype=torch.float64, device=stack.device)
    elif not torch.is_tensor(sums) or sums.dtype != torch.float64 or not sums.is_cuda or sums.numel() != T + 1 or not sums.is_contiguous():
        raise ValueError("frame_dots: sums must be a contiguous float64 [T + 1] device tensor")
    ws = torch.empty(max(int(L.cwfa_frame_dots_workspace_bytes(T, P)) // 8, 1), dtype=torch.float64, device=stack.device)
    check(L.cwfa_frame_dots(_p(stack), dt, T, P, fs, _p(b), _p(sums), _p(ws), acc, _stream()), "frame_dots")
    return sums


def sparse_residual(stack, a, b, tau=None, out=None, pair=False):
    """S = relu(stack - a[t] * b[p] - tau[p]) in separately rounded fp32 operations (``tau`` None: no last subtraction), float32 of
    the stack's shape; ``pair``: the [T, ..., 2] layout with the widened stack in channel 0 and S in channel 1, written in one pass.
    ``out``: a contiguous float32 tensor of that shape; an fp32 contiguous ``stack`` itself works in place (``pair`` False)."""
    L = _lib.lib()
    given = stack
    stack, dt, T, P, fs = _stack(stack, "sparse_residual")
    a, b = _vec(a, T, "a", "sparse_residual"), _vec(b, P, "b", "sparse_residual")
    tau = None if tau is None else _vec(tau, P, "tau", "sparse_residual")
    shape = tuple(stack.shape) + ((2,) if pair else ())
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=stack.device)
    elif not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"sparse_residual: out must be a contiguous float32 {shape} device tensor")
    elif out is given and stack is not given:
        raise ValueError("sparse_residual: in place needs a contiguous stack")
    check(L.cwfa_sparse_residual(_p(stack), dt, T, P, fs, _p(a), _p(b), _p(tau), _p(out), int(bool(pair)), _stream()), "sparse_residual")
    return out


# ------------------------------------------------------------------------------------------------ rigid frame registration
_REG_AXES = {2: ("[N, H, W]", "frame", "(my, mx)"), 3: ("[N, D, H, W]", "volume", "(mz, my, mx)")}


def _by(sides):
    return " x ".join(str(s) for s in sides)


def _reg_stack(x, rank, what):
    """A stack of frames [N, H, W] (``rank`` 2, fp32 / fp16) or of volumes [N, D, H, W] (``rank`` 3, fp32) as ``_stack`` returns it:
    (tensor, dtype code, N, (H, W) or (D, H, W), item stride)."""
    x, dt, N, P, fs = _stack(x, what)
    if rank == 3 and dt != 0:
        raise TypeError(f"{what}: float32 volumes are expected, got {x.dtype}")
    if x.dim() != rank + 1:
        raise ValueError(f"{what}: a stack {_REG_AXES[rank][0]} is expected, got {tuple(x.shape)}")
    shape = tuple(x.shape[1:])
    if P >= 1 << 31:
        raise ValueError(f"{what}: a {_REG_AXES[rank][1]} of {_by(shape)} is too large")
    return x, dt, N, shape, fs


def _overlap(a, b):
    """Whether two tensors share bytes of one storage (bounds of the views, conservative)."""
    if a.numel() == 0 or b.numel() == 0 or a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
        return False
    span = lambda t: (t.data_ptr(), t.data_ptr() + (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size())
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def _reg_out(out, shape, dtype, word, what, like, alias=True):
    """``out`` of a registration pass: a new tensor of ``shape`` and ``dtype`` on the device of ``like``, or the given one, which
    must be that, contiguous, and (``alias``) share no memory with ``like``, the stack.  ``word``: the dtype as the message names it."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if not torch.is_tensor(out) or not out.is_cuda or out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous {word} {shape} device tensor")
    if alias and _overlap(out, like):
        raise ValueError(f"{what}: out must not alias the stack")
    return out


def _reg_window(stack, w, out, what):
    """``reg_window`` (two vectors) and ``reg_window3d`` (three): one kernel, a frame being a volume of one plane."""
    L = _lib.lib()
    stack, dt, N, shape, fs = _reg_stack(stack, len(w), what)
    w = [_vec(v, n, name, what) for v, n, name in zip(w, shape, ("wz", "wy", "wx")[3 - len(w):])]
    out = _reg_out(out, (N, *shape), torch.float32, "float32", what, stack)
    if len(w) == 2:
        check(L.cwfa_reg_window(_p(stack), dt, N, *shape, fs, _p(w[0]), _p(w[1]), _p(out), _stream()), what)
    else:
        check(L.cwfa_reg_window3d_f32(_p(stack), N, *shape, fs, _p(w[0]), _p(w[1]), _p(w[2]), _p(out), _stream()), what)
    return out


def reg_window(stack, wy, wx, out=None):
    """float32 [N,H,W]: fl(float(stack) * fl(wy[y] * wx[x])) for a [N,H,W] fp32 / fp16 device stack and fp32 device vectors ``wy``
    [H], ``wx`` [W] -- the edge taper in front of the forward transform, with the widening of an fp16 stack, in one read and one
    write.  ``out``: a contiguous float32 tensor of the stack's shape that shares no memory with it."""
    return _reg_window(stack, (wy, wx), out, "reg_window")


def reg_whiten(F, W=None, eps=1e-5, out=None):
    """F / (|F| + eps) for a contiguous complex64 device tensor, times the complex64 weight plane ``W`` where one is given: ``W``
    has the shape of F's trailing axes and is shared by everything in front of them.  Each factor is whitened on its own: the
    modulus of a product of two spectra overflows fp32 where the factors' do not.  ``out``: F itself (in place) or a contiguous
    complex64 tensor of its shape."""
    L = _lib.lib()
    _cdev(F, "reg_whiten")
    eps = float(eps)
    if not 0.0 <= eps < float("inf"):
        raise ValueError(f"reg_whiten: eps must be finite and not negative, got {eps}")
    if W is None:
        N, bins = 1, F.numel()
    else:
        _cdev(W, "reg_whiten: W")
        if W.dim() > F.dim() or tuple(F.shape[F.dim() - W.dim():]) != tuple(W.shape):
            raise ValueError(f"reg_whiten: W {tuple(W.shape)} is not the trailing shape of F {tuple(F.shape)}")
        bins = W.numel()
        N = F.numel() // bins if bins else 0
        if _overlap(W, F) or (out is not None and torch.is_tensor(out) and _overlap(W, out)):
            raise ValueError("reg_whiten: W must not alias F or out")
    if out is None:
        out = torch.empty_like(F)
    elif out is not F:
        _cdev(out, "reg_whiten: out")
        if tuple(out.shape) != tuple(F.shape):
            raise ValueError(f"reg_whiten: out must have F's shape {tuple(F.shape)}")
        if _overlap(out, F) and out.data_ptr() != F.data_ptr():
            raise ValueError("reg_whiten: out is F itself or shares no memory with it")
    check(L.cwfa_reg_whiten_c64(_p(F), _p(W), N, bins, eps, _p(out), _stream()), "reg_whiten")
    return out


def _max_shift(max_shift, *sides_and_what):
    """``_max_shift(max_shift, H, W, what)`` or ``(max_shift, D, H, W, what)``: an int or one bound per axis, as a tuple."""
    shape, what = sides_and_what[:-1], sides_and_what[-1]
    try:
        m = (max_shift,) * len(shape) if isinstance(max_shift, int) else tuple(max_shift)
        if len(m) != len(shape):
            raise TypeError
        m = tuple(map(int, m))
    except TypeError:
        raise ValueError(f"{what}: max_shift is an int or {_REG_AXES[len(shape)][2]}, got {max_shift!r}") from None
    fits = 0 not in shape
    for v, n in zip(m, shape):
        if v < 0 or (fits and 2 * v + 1 > n):
            raise ValueError(f"{what}: max_shift ({', '.join(map(str, m))}) needs 0 <= 2 m + 1 <= the {_REG_AXES[len(shape)][1]}'s {_by(shape)}")
    return m


_max_shift3 = _max_shift          # the name the volume side grew up with


def _reg_peak(corr, max_shift, subpixel, out, rank, what):
    """``reg_peak`` (``rank`` 2) and ``reg_peak3d`` (3): the checks and the call; the kernels are two over one key order."""
    L = _lib.lib()
    corr, dt, N, shape, fs = _reg_stack(corr, rank, what)
    if dt != 0:
        raise TypeError(f"{what}: float32 correlation maps are expected")
    m = _max_shift(max_shift, *shape, what)
    if out is None:
        out = (torch.empty((N, rank), dtype=torch.float32, device=corr.device), torch.empty((N, rank), dtype=torch.int32, device=corr.device),
               torch.empty((N,), dtype=torch.float32, device=corr.device))
    shifts, ipeak, peak = out
    for t, dtype, tshape, name in ((shifts, torch.float32, (N, rank), "shifts"), (ipeak, torch.int32, (N, rank), "ipeak"), (peak, torch.float32, (N,), "peak")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != tshape or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous {dtype} {tshape} device tensor")
    fn = L.cwfa_reg_peak_f32 if rank == 2 else L.cwfa_reg_peak3d_f32
    check(fn(_p(corr), N, *shape, fs, *m, int(bool(subpixel)), _p(shifts), _p(ipeak), _p(peak), _stream()), what)
    return shifts, ipeak, peak


def reg_peak(corr, max_shift, subpixel=True, out=None):
    """(shifts float32 [N,2], ipeak int32 [N,2], peak float32 [N]) on the device from float32 correlation maps [N,H,W]: the maximum
    over the signed window |sy| <= my, |sx| <= mx (read modulo the frame) under the total order of ``local_maxima`` -- ties to the
    lowest window index, NaN below everything -- and, with ``subpixel``, a parabola per axis through the peak and its two
    neighbours in float64.  A window without a finite value gives shift (0, 0) and peak NaN.  ``out``: the three tensors."""
    return _reg_peak(corr, max_shift, subpixel, out, 2, "reg_peak")


def reg_roots(M):
    """float64 [M, 2] on the CPU: (cos, sin)(2 pi k / M), k = 0 .. M - 1, the root table of ``reg_upsample``.  The angle is reduced
    to the first octant in integers -- pi p / q with p = 2 k, q = M, mirrored at pi, pi / 2 and pi / 4 -- and only then formed in
    float64 as fl(fl(pi * p) / q); ``math.cos`` and ``math.sin`` of that, swapped and signed by the mirrors."""
    import math
    M = int(M)
    rows = []
    for k in range(M):
        p, q, sc, ss = 2 * k, M, 1.0, 1.0
        if p > q:
            p, ss = 2 * q - p, -1.0
        if 2 * p > q:
            p, sc = q - p, -1.0
        swap = 4 * p > q
        if swap:
            p, q = q - 2 * p, 2 * q
        t = math.pi * p / q
        c, s = (math.sin(t), math.cos(t)) if swap else (math.cos(t), math.sin(t))
        rows.append((sc * c, ss * s))
    return torch.tensor(rows, dtype=torch.float64).reshape(M, 2)


_REG_ROOTS = {}


def _reg_roots_dev(M, device):
    key = (int(M), str(device))
    if key not in _REG_ROOTS:
        if len(_REG_ROOTS) >= 8:
            _REG_ROOTS.clear()
        _REG_ROOTS[key] = reg_roots(M).to(device)
    return _REG_ROOTS[key]


def _count(v, name, what):
    """An integer of at least 1 (bool and float refused)."""
    import operator
    try:
        if isinstance(v, bool):
            raise TypeError
        n = operator.index(v)
    except TypeError:
        raise ValueError(f"{what}: {name} must be an integer, got {v!r}") from None
    if n < 1:
        raise ValueError(f"{what}: {name} must be at least 1, got {n}")
    return n


def _fine_grid(upsample, radius, what):
    u = _count(upsample, "upsample", what)
    r = u if radius is None else _count(radius, "radius", what)
    if r >= 1 << 14:
        raise ValueError(f"{what}: radius = {r} is too large")
    return u, r


def _ipeak(ipeak, N, what):
    if not torch.is_tensor(ipeak) or ipeak.dtype != torch.int32 or tuple(ipeak.shape) != (N, 2) or not ipeak.is_contiguous():
        raise ValueError(f"{what}: ipeak must be a contiguous int32 {(N, 2)} tensor")
    if not ipeak.is_cuda:
        raise RuntimeError(f"{what}: cwfa_amd runs on MI355X only -- ipeak is a {ipeak.device} tensor (no CPU fallback exists)")
    return ipeak


def reg_upsample(R, ipeak, shape, upsample, radius=None, out=None, workspace=None):
    """float64 [N, U, U], U = 2 ``radius`` + 1: the correlation irfft2(R, s=shape) interpolated trigonometrically on the fine grid
    y = py + j / ``upsample``, x = px + j / ``upsample``, j = -radius .. radius, around the integer peaks ``ipeak`` (int32 [N,2], as
    ``reg_peak`` writes them), straight from the spectra R (complex64 [N, H, W/2+1], frames contiguous, any stride between them): an
    up-sampled DFT in float64 with a fixed summation order.  ``radius`` None: ``upsample``, i.e. +-1 px.
    ``out``: a contiguous float64 [N,U,U] device tensor.  ``workspace``: a device tensor of at least
    ``cwfa_reg_upsample_workspace_bytes`` bytes, 16-byte aligned."""
    what = "reg_upsample"
    u, r = _fine_grid(upsample, radius, what)
    if not isinstance(shape, (tuple, list, torch.Size)) or len(shape) != 2:
        raise ValueError(f"{what}: shape is (H, W), got {shape!r}")
    H, W = (_count(s, "shape", what) for s in shape)
    if not torch.is_tensor(R):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(R)}")
    if R.dtype != torch.complex64:
        raise TypeError(f"{what}: expected complex64 spectra, got {R.dtype}")
    if R.dim() != 3 or tuple(R.shape[1:]) != (H, W // 2 + 1):
        raise ValueError(f"{what}: R {tuple(R.shape)} is not [N, {H}, {W // 2 + 1}], the spectra of {H} x {W} frames")
    if H * W >= 1 << 31 or H * u >= 1 << 31 or W * u >= 1 << 31:
        raise ValueError(f"{what}: {H} x {W} at factor {u} is too large")
    N, K, U = int(R.shape[0]), W // 2 + 1, 2 * r + 1
    ipeak = _ipeak(ipeak, N, what)
    if not R.is_cuda:
        raise RuntimeError(f"{what}: cwfa_amd runs on MI355X only -- got a {R.device} tensor (no CPU fallback exists)")
    if N and (not R[0].is_contiguous() or (N > 1 and R.stride(0) < H * K)):
        R = R.contiguous()
    fs = R.stride(0) if N > 1 else H * K
    out = _reg_out(out, (N, U, U), torch.float64, "float64", what, R, alias=False)
    if N == 0:
        return out
    L = _lib.lib()
    nbytes = int(L.cwfa_reg_upsample_workspace_bytes(N, H, W, r))
    if nbytes < 0:
        raise ValueError(f"{what}: {H} x {W} at radius {r} is too large")
    if workspace is None:
        workspace = torch.empty(max(nbytes // 8, 2), dtype=torch.float64, device=R.device)
    elif not torch.is_tensor(workspace) or not workspace.is_cuda or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError(f"{what}: workspace must be a contiguous device tensor of at least {nbytes} bytes")
    check(L.cwfa_reg_upsample_c64(_p(R), N, H, W, fs, _p(ipeak), u, r, _p(_reg_roots_dev(W * u, R.device)), _p(_reg_roots_dev(H * u, R.device)),
                                  _p(out), _p(workspace), _stream()), what)
    return out


def reg_fine_peak(C, ipeak, upsample, out=None):
    """(shifts float32 [N,2], peak float32 [N]) on the device from the fine maps ``C`` (float64 [N,U,U] of ``reg_upsample``) and the
    integer peaks: the maximum of every map under the order of ``reg_peak`` widened to 64 bits, a float64 parabola per axis through
    it and its two fine neighbours where it is not on the grid's border, shift = ipeak + (j + delta) / ``upsample``.  A map without
    a finite value gives the integer peak and peak NaN.  ``out``: the two tensors as ``reg_peak`` filled them -- a frame whose peak
    is NaN there is left as it is."""
    what = "reg_fine_peak"
    u = _count(upsample, "upsample", what)
    if not torch.is_tensor(C):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(C)}")
    if C.dtype != torch.float64:
        raise TypeError(f"{what}: expected float64 maps, got {C.dtype}")
    if C.dim() != 3 or C.shape[1] != C.shape[2] or C.shape[1] < 3 or C.shape[1] % 2 == 0 or C.shape[1] >= 1 << 15 or not C.is_contiguous():
        raise ValueError(f"{what}: C {tuple(C.shape)} is not a contiguous [N, U, U] with U = 2 r + 1, r >= 1")
    N, U = int(C.shape[0]), int(C.shape[1])
    ipeak = _ipeak(ipeak, N, what)
    if not C.is_cuda:
        raise RuntimeError(f"{what}: cwfa_amd runs on MI355X only -- got a {C.device} tensor (no CPU fallback exists)")
    keep = out is not None
    if out is None:
        out = (torch.empty((N, 2), dtype=torch.float32, device=C.device), torch.empty((N,), dtype=torch.float32, device=C.device))
    shifts, peak = out
    for t, shape, name in ((shifts, (N, 2), "shifts"), (peak, (N,), "peak")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous float32 {shape} device tensor")
    if N == 0:
        return shifts, peak
    check(_lib.lib().cwfa_reg_fine_peak_f64(_p(C), _p(ipeak), N, U, u, int(keep), _p(shifts), _p(peak), _stream()), what)
    return shifts, peak


def _shift_mode(mode, what, plain=False):
    """The entry points' code of ``mode``.  ``plain``: the message names the modes as the functions of CWFA.py and XLFMDataset.py do."""
    if mode not in _lib.SHIFT_MODE:
        names = " or ".join(repr(m) for m in sorted(_lib.SHIFT_MODE)) if plain else f"one of {sorted(_lib.SHIFT_MODE)}"
        raise ValueError(f"{what}: mode is {names}, got {mode!r}")
    return _lib.SHIFT_MODE[mode]


def _reg_shift(stack, shifts, mode, fill, out, rank, what):
    """``reg_shift`` (``rank`` 2) and ``reg_shift3d`` (3): the checks and the call; the kernels are two (the z walk is the volumes')."""
    L = _lib.lib()
    stack, dt, N, shape, fs = _reg_stack(stack, rank, what)
    mode = _shift_mode(mode, what)
    shifts = _vec(shifts, rank * N, "shifts", what)
    out = _reg_out(out, (N, *shape), stack.dtype, stack.dtype if rank == 2 else "float32", what, stack)
    args = (fs, _p(shifts), mode, float(fill), _p(out), _stream())
    check(L.cwfa_reg_shift(_p(stack), dt, N, *shape, *args) if rank == 2 else L.cwfa_reg_shift3d_f32(_p(stack), N, *shape, *args), what)
    return out


def reg_shift(stack, shifts, mode="bilinear", fill=0.0, out=None):
    """out[n,y,x] = stack[n, y + dy, x + dx] with (dy, dx) = shifts[n] read on the device (float32 [N,2]): bilinear with separately
    rounded fp32 weights and products, or ``mode="nearest"`` (rintf of the shift).  A tap of weight exactly 0 is neither read nor
    added, so an integer shift copies bits; a tap outside the frame reads ``fill``; a non-finite shift fills the frame.  The result
    has the stack's dtype.  ``out``: a contiguous tensor of the stack's shape and dtype that shares no memory with it."""
    return _reg_shift(stack, shifts, mode, fill, out, 2, "reg_shift")


# ------------------------------------------------------------------------------------------------ per-lenslet registration
def _view_centers(centers, view_shape, what):
    """(int32 [L,2] host table, ph, pw): the lenslet centres (row, column) as the entry points take them, 1 <= L <= 254."""
    import numpy as np
    if torch.is_tensor(centers):
        centers = centers.detach().cpu().numpy()
    try:
        c = np.asarray(centers)
        ok = np.issubdtype(c.dtype, np.integer) and c.ndim == 2 and c.shape[1] == 2
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: centers is an integer [L,2] table of (row, column)")
    if not 1 <= len(c) <= _lib.REG_MAX_VIEWS:
        raise ValueError(f"{what}: 1 to {_lib.REG_MAX_VIEWS} views are expected, got {len(c)}")
    if (np.abs(c.astype(np.int64)) >= 1 << 29).any():
        raise ValueError(f"{what}: a centre is out of range")
    if not isinstance(view_shape, (tuple, list, torch.Size)) or len(view_shape) != 2:
        raise ValueError(f"{what}: view_shape is (ph, pw), got {view_shape!r}")
    ph, pw = (_count(s, "view_shape", what) for s in view_shape)
    if ph * pw >= 1 << 31:
        raise ValueError(f"{what}: a view of {ph} x {pw} is too large")
    return np.ascontiguousarray(c.astype(np.int32)), ph, pw


def reg_window_views(stack, centers, view_shape, wy, wx, out=None):
    """float32 [N,L,ph,pw]: the L views of every frame of a [N,H,W] fp32 / fp16 device stack, cut, widened and tapered in one read:
    fl(float(stack[n, cy - ph//2 + y, cx - pw//2 + x]) * fl(wy[y] * wx[x])), a pixel outside the frame read as 0.  ``centers``: an
    integer [L,2] HOST table of (row, column), 1 <= L <= 254; ``wy`` [ph], ``wx`` [pw] fp32 device vectors.  For even sizes the box is
    that of ``extract_views``; odd sizes differ (``extract_views`` returns 2 (s // 2)).  ``out``: a contiguous float32 tensor of that
    shape that shares no memory with the stack."""
    what = "reg_window_views"
    c, ph, pw = _view_centers(centers, view_shape, what)
    stack, dt, N, (H, W), fs = _reg_stack(stack, 2, what)
    if H < 1 or W < 1:
        raise ValueError(f"{what}: a frame of {H} x {W}")
    wy, wx = _vec(wy, ph, "wy", what), _vec(wx, pw, "wx", what)
    out = _reg_out(out, (N, len(c), ph, pw), torch.float32, "float32", what, stack)
    if N == 0:
        return out
    check(_lib.lib().cwfa_reg_window_views(_p(stack), dt, N, H, W, fs, _host(c), len(c), ph, pw, _p(wy), _p(wx), _p(out), _stream()), what)
    return out


def reg_label_map(shape, centers, view_shape, device="cuda"):
    """uint8 [H,W] on ``device``: the index of the view whose box holds the pixel -- among several boxes the one whose centre is
    nearest in integer squared distance, ties to the lowest index -- and L, "the rest of the frame", where none does."""
    what = "reg_label_map"
    c, ph, pw = _view_centers(centers, view_shape, what)
    if not isinstance(shape, (tuple, list, torch.Size)) or len(shape) != 2:
        raise ValueError(f"{what}: shape is (H, W), got {shape!r}")
    H, W = (_count(s, "shape", what) for s in shape)
    if H * W >= 1 << 31:
        raise ValueError(f"{what}: a frame of {H} x {W} is too large")
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"{what}: cwfa_amd runs on MI355X only -- got device {device!r} (no CPU fallback exists)")
    L = _lib.lib()
    labels = torch.empty((H, W), dtype=torch.uint8, device=device)
    check(L.cwfa_reg_label_map(_host(c), len(c), ph, pw, H, W, _p(labels), _stream()), what)
    return labels


def reg_fit_views(shifts, peak, directions, min_peak=0.0, reject=1.0, model="axial"):
    """(table float32 [N,L+1,2], params float64 [N,3], inlier uint8 [N,L]) on the device from the per-view shifts (float32 [N,L,2]),
    their peaks (float32 [N,L]) and the directions g (float64 [L,2]): per frame the least-squares fit s_i = d + a g_i over the views
    whose peak is finite and >= ``min_peak``, one rejection pass at ``reject`` pixels (inf: none) and a second fit, in float64 with a
    fixed summation order.  ``params`` = (d_y, d_x, a).  Row L of ``table`` is d; row i is d + a g_i
    (``model="axial"``) or the measured s_i where ``inlier`` and the model value where not (``"free"``)."""
    what = "reg_fit_views"
    if model not in _lib.VIEW_MODEL:
        raise ValueError(f"{what}: model is one of {sorted(_lib.VIEW_MODEL)}, got {model!r}")
    min_peak, reject = float(min_peak), float(reject)
    if not min_peak >= 0.0 or not reject >= 0.0:
        raise ValueError(f"{what}: min_peak and reject are not negative and not NaN, got {min_peak}, {reject}")
    if not torch.is_tensor(shifts) or shifts.dim() != 3 or shifts.shape[2] != 2:
        raise ValueError(f"{what}: shifts is a float32 [N,L,2] tensor")
    N, Lv = int(shifts.shape[0]), int(shifts.shape[1])
    if not 1 <= Lv <= _lib.REG_MAX_VIEWS:
        raise ValueError(f"{what}: 1 to {_lib.REG_MAX_VIEWS} views are expected, got {Lv}")
    shifts, peak = _vec(shifts, 2 * N * Lv, "shifts", what), _vec(peak, N * Lv, "peak", what)
    directions = _vec(directions, 2 * Lv, "directions", what, torch.float64)
    dev = shifts.device
    table = torch.empty((N, Lv + 1, 2), dtype=torch.float32, device=dev)
    params = torch.empty((N, 3), dtype=torch.float64, device=dev)
    inlier = torch.empty((N, Lv), dtype=torch.uint8, device=dev)
    if N == 0:
        return table, params, inlier
    check(_lib.lib().cwfa_reg_fit_views_f64(_p(shifts), _p(peak), _p(directions), N, Lv, min_peak, reject, _lib.VIEW_MODEL[model], _p(params),
                                            _p(inlier), _p(table), _stream()), what)
    return table, params, inlier


def reg_shift_labeled(stack, table, labels, mode="bilinear", fill=0.0, out=None):
    """``reg_shift`` with a shift per pixel label: out[n,y,x] = stack[n, y + dy, x + dx], (dy, dx) = table[n, min(labels[y,x], L)]
    read on the device (``table`` float32 [N,L+1,2], ``labels`` uint8 [H,W]).  Taps, weights, order, ``fill`` and dtype are those of
    ``reg_shift``, bit for bit; the source is the whole frame, so a tap that leaves its view's box reads what lies there.  ``out``: a
    contiguous tensor of the stack's shape and dtype that shares no memory with it."""
    what = "reg_shift_labeled"
    stack, dt, N, (H, W), fs = _reg_stack(stack, 2, what)
    mode = _shift_mode(mode, what)
    if not torch.is_tensor(table) or table.dim() != 3 or int(table.shape[0]) != N or table.shape[2] != 2 or not 2 <= table.shape[1] <= _lib.REG_MAX_VIEWS + 1:
        raise ValueError(f"{what}: table is a float32 [{N}, L + 1, 2] tensor, 1 <= L <= {_lib.REG_MAX_VIEWS}")
    Lv = int(table.shape[1]) - 1
    table = _vec(table, 2 * N * (Lv + 1), "table", what)
    labels = _vec(labels, H * W, "labels", what, torch.uint8)
    if H < 1 or W < 1:
        raise ValueError(f"{what}: a frame of {H} x {W}")
    out = _reg_out(out, (N, H, W), stack.dtype, stack.dtype, what, stack)
    if N == 0:
        return out
    check(_lib.lib().cwfa_reg_shift_labeled(_p(stack), dt, N, H, W, fs, _p(table), _p(labels), Lv, mode, float(fill), _p(out),
                                            _stream()), what)
    return out


# ------------------------------------------------------------------------------------------------ registration of volumes
def reg_window3d(stack, wz, wy, wx, out=None):
    """float32 [N,D,H,W]: fl(stack * fl(fl(wz[z] * wy[y]) * wx[x])) for a [N,D,H,W] float32 device stack and float32 device vectors
    ``wz`` [D], ``wy`` [H], ``wx`` [W] -- the edge taper in front of the forward transform, in one read and one write.  ``out``: a
    contiguous float32 tensor of the stack's shape that shares no memory with it."""
    return _reg_window(stack, (wz, wy, wx), out, "reg_window3d")


def reg_peak3d(corr, max_shift, subpixel=True, out=None):
    """(shifts float32 [N,3] as (dz, dy, dx), ipeak int32 [N,3], peak float32 [N]) on the device from float32 correlation maps
    [N,D,H,W]: ``reg_peak`` with one more axis -- the maximum over the signed window |sz| <= mz, |sy| <= my, |sx| <= mx (read modulo
    the volume; ``max_shift``: an int or (mz, my, mx)), ties to the lowest window index, NaN below everything, and with ``subpixel``
    a float64 parabola per axis.  A window without a finite value gives shift 0 and peak NaN.  ``out``: the three tensors."""
    return _reg_peak(corr, max_shift, subpixel, out, 3, "reg_peak3d")


def reg_shift3d(stack, shifts, mode="bilinear", fill=0.0, out=None):
    """out[n,z,y,x] = stack[n, z + dz, y + dy, x + dx] with (dz, dy, dx) = shifts[n] read on the device (float32 [N,3]): ``reg_shift``
    of the planes z + floor(dz) and the next one under (dy, dx), blended along z with separately rounded fp32 weights and products;
    ``mode="nearest"``: rintf of the shift.  A plane or tap of weight exactly 0 is neither read nor added, so an integer shift
    copies bits; whatever lies outside the volume reads ``fill``; a non-finite shift fills the volume.  ``out``: a contiguous
    float32 tensor of the stack's shape that shares no memory with it."""
    return _reg_shift(stack, shifts, mode, fill, out, 3, "reg_shift3d")


# ------------------------------------------------------------------------------------------------ piecewise-rigid registration of volumes
def _block_grid3(grid, what):
    """(gz, gy, gx): three counts of at least 1 whose product is at most ``REG_MAX_BLOCKS``."""
    if not isinstance(grid, (tuple, list, torch.Size)) or len(grid) != 3:
        raise ValueError(f"{what}: grid is (gz, gy, gx), got {grid!r}")
    g = tuple(_count(v, "grid", what) for v in grid)
    if g[0] * g[1] * g[2] > _lib.REG_MAX_BLOCKS:
        raise ValueError(f"{what}: a grid of {_by(g)} has more than {_lib.REG_MAX_BLOCKS} blocks")
    return g


def _block_origins(origins, block, shape, what):
    """(int32 host table [gz + gy + gx], (gz, gy, gx), (bz, by, bx)): the origins per axis, every block inside the volume."""
    import numpy as np
    if not isinstance(block, (tuple, list, torch.Size)) or len(block) != 3:
        raise ValueError(f"{what}: block is (bz, by, bx), got {block!r}")
    b = tuple(_count(v, "block", what) for v in block)
    if any(v > s for v, s in zip(b, shape)):
        raise ValueError(f"{what}: a block of {_by(b)} does not fit the {_by(shape)} volume")
    if not isinstance(origins, (tuple, list)) or len(origins) != 3:
        raise ValueError(f"{what}: origins is three integer sequences, one per axis")
    rows = []
    for a, o in enumerate(origins):
        try:
            o = np.asarray(o.detach().cpu().numpy() if torch.is_tensor(o) else o)
            ok = o.ndim == 1 and o.size >= 1 and np.issubdtype(o.dtype, np.integer)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{what}: origins[{a}] is a sequence of at least one integer")
        if (o < 0).any() or (o.astype(np.int64) > shape[a] - b[a]).any():
            raise ValueError(f"{what}: an origin of axis {a} puts the block outside the volume")
        rows.append(o.astype(np.int32))
    g = _block_grid3(tuple(len(r) for r in rows), what)
    return np.ascontiguousarray(np.concatenate(rows)), g, b


def reg_window_blocks3d(stack, origins, block, wz, wy, wx, out=None):
    """float32 [N,B,bz,by,bx]: the gz x gy x gx blocks of every volume of a [N,D,H,W] float32 device stack, cut and tapered in one
    read: fl(stack[n, oz + z, oy + y, ox + x] * fl(fl(wz[z] * wy[y]) * wx[x])), block (iz gy + iy) gx + ix.  ``origins``: three HOST
    integer sequences (z, y, x; their lengths are the grid, at most 4096 blocks) that keep every block of ``block`` = (bz, by, bx)
    inside the volume; ``wz`` [bz], ``wy`` [by], ``wx`` [bx] fp32 device vectors.  ``out``: a contiguous float32 tensor of that
    shape that shares no memory with the stack."""
    what = "reg_window_blocks3d"
    if not torch.is_tensor(stack) or stack.dim() != 4:
        raise ValueError(f"{what}: a stack {_REG_AXES[3][0]} is expected")
    o, g, b = _block_origins(origins, block, tuple(int(s) for s in stack.shape[1:]), what)      # the host table first: no device needed
    stack, _, N, shape, fs = _reg_stack(stack, 3, what)
    w = [_vec(v, n, name, what) for v, n, name in zip((wz, wy, wx), b, ("wz", "wy", "wx"))]
    out = _reg_out(out, (N, g[0] * g[1] * g[2], *b), torch.float32, "float32", what, stack)
    if N == 0:
        return out
    check(_lib.lib().cwfa_reg_window_blocks3d_f32(_p(stack), N, *shape, fs, _host(o), *g, *b, _p(w[0]), _p(w[1]), _p(w[2]), _p(out), _stream()), what)
    return out


def reg_field_fill(shifts, peak, base, grid, min_peak=0.0, max_dev=None, out=None):
    """(field float32 [N,B,3], inlier uint8 [N,B]) on the device: the one clean-up pass over the table of block shifts (float32
    [N,B,3], B = gz gy gx of ``grid``) with their peaks (float32 [N,B]) and a base shift per volume (float32 [N,3]).  A node is an
    inlier when its peak is finite and >= ``min_peak``, its components are finite and |s_c - base_c| <= ``max_dev``[c] (three
    numbers; None: no such test), compared in float64; an inlier keeps its bits, an outlier takes per component the float64 mean of
    the inliers among its 26 grid neighbours (fixed order, status read from the input) rounded once, or ``base`` where it has none.
    ``out``: the two tensors; ``field`` must not be ``shifts``."""
    import ctypes
    what = "reg_field_fill"
    g = _block_grid3(grid, what)
    B = g[0] * g[1] * g[2]
    min_peak = float(min_peak)
    if min_peak != min_peak:
        raise ValueError(f"{what}: min_peak is NaN")
    md = None
    if max_dev is not None:
        try:
            md = tuple(float(v) for v in max_dev)
        except (TypeError, ValueError):
            md = ()
        if len(md) != 3 or not all(v >= 0.0 for v in md):
            raise ValueError(f"{what}: max_dev is None or three numbers that are not negative and not NaN, got {max_dev!r}")
    if not torch.is_tensor(shifts) or shifts.dim() != 3 or int(shifts.shape[1]) != B or shifts.shape[2] != 3:
        raise ValueError(f"{what}: shifts is a float32 [N, {B}, 3] tensor")
    N = int(shifts.shape[0])
    shifts, peak, base = _vec(shifts, 3 * N * B, "shifts", what), _vec(peak, N * B, "peak", what), _vec(base, 3 * N, "base", what)
    dev = shifts.device
    if out is None:
        out = (torch.empty((N, B, 3), dtype=torch.float32, device=dev), torch.empty((N, B), dtype=torch.uint8, device=dev))
    field, inlier = out
    for t, dtype, tshape, name in ((field, torch.float32, (N, B, 3), "field"), (inlier, torch.uint8, (N, B), "inlier")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != tshape or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous {dtype} {tshape} device tensor")
    if _overlap(field, shifts):
        raise ValueError(f"{what}: field must not alias shifts")
    if N == 0:
        return field, inlier
    mdp = None if md is None else (ctypes.c_double * 3)(*md)
    check(_lib.lib().cwfa_reg_field_fill(_p(shifts), _p(peak), _p(base), N, *g, min_peak, mdp, _p(field), _p(inlier), _stream()), what)
    return field, inlier


def reg_warp3d(stack, field, grid, tables, mode="bilinear", fill=0.0, out=None):
    """out[n,z,y,x] = stack[n, z + dz, y + dy, x + dx] with (dz, dy, dx) the trilinear interpolation of the node table ``field``
    (float32 [N,B,3], B = gz gy gx of ``grid``) at the voxel: ``tables`` = (idxz, tz, idxy, ty, idxx, tx), device vectors over the
    coordinates of each axis (int32 node at or below, float32 fraction towards the next, as ``CWFA.block_grid`` makes them), lerp
    a + t (b - a) along x, then y, then z, every operation rounded, t == 0 taking a itself.  The resampling of a voxel is that of
    ``reg_shift3d`` under its vector, bit for bit, so a field whose nodes are equal gives ``reg_shift3d``.  ``out``: a contiguous
    float32 tensor of the stack's shape that shares no memory with it."""
    what = "reg_warp3d"
    mode = _shift_mode(mode, what)
    g = _block_grid3(grid, what)
    if not isinstance(tables, (tuple, list)) or len(tables) != 6:
        raise ValueError(f"{what}: tables is (idxz, tz, idxy, ty, idxx, tx)")
    stack, _, N, shape, fs = _reg_stack(stack, 3, what)
    B = g[0] * g[1] * g[2]
    if not torch.is_tensor(field) or field.dim() != 3 or tuple(field.shape) != (N, B, 3):
        raise ValueError(f"{what}: field is a float32 [{N}, {B}, 3] tensor")
    field = _vec(field, 3 * N * B, "field", what)
    tabs = []
    for k, (t, name) in enumerate(zip(tables, ("idxz", "tz", "idxy", "ty", "idxx", "tx"))):
        tabs.append(_vec(t, shape[k // 2], name, what, torch.float32 if k & 1 else torch.int32))
    out = _reg_out(out, (N, *shape), torch.float32, "float32", what, stack)
    if N == 0:
        return out
    check(_lib.lib().cwfa_reg_warp3d_f32(_p(stack), N, *shape, fs, _p(field), *g, *(_p(t) for t in tabs), mode, float(fill), _p(out),
                                         _stream()), what)
    return out


# ------------------------------------------------------------------------------------------------ rigid registration with a rotation about z
def _rigid_center(center, shape, what):
    """(cy, cx): two finite floats, the centre of the plane where ``center`` is None."""
    if center is None:
        return (shape[-2] - 1) / 2.0, (shape[-1] - 1) / 2.0
    try:
        c = tuple(float(v) for v in center)
    except (TypeError, ValueError):
        c = ()
    if len(c) != 2 or not all(abs(v) < float("inf") for v in c):
        raise ValueError(f"{what}: center is None or two finite numbers (cy, cx), got {center!r}")
    return c


def reg_fit_rigid(shifts, peak, arms, min_peak=0.0, reject=1.0, prior=None):
    """(params float64 [N,5], inlier uint8 [N,B]) on the device from a table of block shifts (float32 [N,B,3]), their peaks (float32
    [N,B]) and the arms (float64 [B,2]: block centre minus rotation centre, (y, x)): per volume the rigid motion (dz, dy, dx, c, s),
    rotation about z by the angle of cosine c and sine s plus a 3-D shift, fitted in float64 with a fixed summation order over the
    blocks whose peak is finite and >= ``min_peak`` and whose shift is finite, one rejection pass at ``reject`` voxels (inf: none) and
    a second fit.  ``prior`` float64 [N,5]: the motion already applied to the measured volumes; the result
    is then the total motion of the original."""
    what = "reg_fit_rigid"
    min_peak, reject = float(min_peak), float(reject)
    if not min_peak >= 0.0 or not reject >= 0.0:
        raise ValueError(f"{what}: min_peak and reject are not negative and not NaN, got {min_peak}, {reject}")
    if not torch.is_tensor(shifts) or shifts.dim() != 3 or shifts.shape[2] != 3:
        raise ValueError(f"{what}: shifts is a float32 [N,B,3] tensor")
    N, B = int(shifts.shape[0]), int(shifts.shape[1])
    if not 1 <= B <= _lib.REG_MAX_BLOCKS:
        raise ValueError(f"{what}: 1 to {_lib.REG_MAX_BLOCKS} blocks are expected, got {B}")
    shifts, peak = _vec(shifts, 3 * N * B, "shifts", what), _vec(peak, N * B, "peak", what)
    arms = _vec(arms, 2 * B, "arms", what, torch.float64)
    if prior is not None:
        prior = _vec(prior, 5 * N, "prior", what, torch.float64)
    dev = shifts.device
    params = torch.empty((N, 5), dtype=torch.float64, device=dev)
    inlier = torch.empty((N, B), dtype=torch.uint8, device=dev)
    if N == 0:
        return params, inlier
    check(_lib.lib().cwfa_reg_fit_rigid_f64(_p(shifts), _p(peak), _p(arms), N, B, min_peak, reject, _p(prior), _p(params), _p(inlier), _stream()), what)
    return params, inlier


def reg_rigid3d(volumes, params, center=None, mode="bilinear", fill=0.0, out=None):
    """out[n,z,y,x] = volumes[n, z + dz, c0 + R ((y, x) - c0) + (dy, dx)] with (dz, dy, dx, c, s) = params[n] read on the device
    (float64 [N,5]), R = [[c, -s], [s, c]] and c0 = ``center`` (cy, cx), None: ((H - 1) / 2, (W - 1) / 2).  The in-plane displacement
    of a voxel is formed in fp32 from (c - 1, s), c - 1 as -(s s) / (1 + c) in float64, and the voxel is resampled as ``reg_shift3d``
    resamples under that vector, bit for bit: (c, s) = (1, 0) gives ``reg_shift3d``, a quarter turn about the centre of a square
    plane copies bits.  A non-finite parameter fills the volume.  ``out``: a contiguous float32 tensor of the stack's shape that
    shares no memory with it."""
    what = "reg_rigid3d"
    mode = _shift_mode(mode, what)
    if not torch.is_tensor(volumes) or volumes.dim() != 4:
        raise ValueError(f"{what}: a stack {_REG_AXES[3][0]} is expected")
    cy, cx = _rigid_center(center, tuple(int(s) for s in volumes.shape), what)
    stack, _, N, shape, fs = _reg_stack(volumes, 3, what)
    if not torch.is_tensor(params) or tuple(params.shape) != (N, 5):
        raise ValueError(f"{what}: params is a float64 [{N}, 5] tensor")
    params = _vec(params, 5 * N, "params", what, torch.float64)
    out = _reg_out(out, (N, *shape), torch.float32, "float32", what, stack)
    if N == 0:
        return out
    check(_lib.lib().cwfa_reg_rigid3d_f32(_p(stack), N, *shape, fs, _p(params), cy, cx, mode, float(fill), _p(out), _stream()), what)
    return out


# ------------------------------------------------------------------------------------------------ neuron footprints
def _nonneg_triple(v, name, what):
    t = _triple(v, name, what)
    if any(a < 0 for a in t):
        raise ValueError(f"{what}: {name} = {t} is negative")
    return t


def _box_table(boxes, name, what, shape=None):
    import numpy as np
    try:
        b = np.asarray(boxes)
        ok = b.size == 0 or (np.issubdtype(b.dtype, np.integer) and b.ndim == 2 and b.shape[1] == 6)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: {name} is an integer [N,6] table (z0, z1, y0, y1, x0, x1)")
    b = np.ascontiguousarray(b.reshape(-1, 6).astype(np.int32))
    if shape is not None:
        lim = np.asarray(shape, dtype=np.int64)
        lo, hi = b[:, 0::2].astype(np.int64), b[:, 1::2].astype(np.int64)
        if ((lo < 0) | (lo > hi) | (hi > lim)).any():
            raise ValueError(f"{what}: every row of {name} is a half-open range inside the volume {tuple(shape)}")
    return b


class FootprintGeometry:
    """The host tables of the footprint passes for ``boxes`` (``roi_boxes``' int32 [N,6]) in volumes of ``shape`` (D, H, W):

    ``cores`` [N,6]: the seed region of every neuron, inside its box; ``shell_outer`` / ``shell_inner`` [N,6]: the box grown by
    ``gap + annulus`` and by ``gap`` per axis and clipped by the volume -- the neuropil shell of neuron n is outer minus inner minus
    every voxel of ``occupancy`` (an empty box has an empty shell); ``offsets`` int64 [N+1]: box n's voxels lie at ``offsets[n]`` of
    the ragged state in the box's own (z, y, x) linear order, ``V = offsets[N]``.  ``occupancy``: uint8 [D,H,W] on ``device``, 1 inside
    any box, marked once on first use.  The tables themselves travel in the kernels' arguments: nothing else is uploaded."""

    def __init__(self, boxes, cores, shape, gap=(1, 2, 2), annulus=(2, 4, 4), device="cuda"):
        import numpy as np
        what = "footprint_geometry"
        shape = tuple(int(s) for s in shape)
        if len(shape) != 3 or min(shape) < 0:
            raise ValueError(f"{what}: shape is (D, H, W), got {shape!r}")
        gap, annulus = _nonneg_triple(gap, "gap", what), _nonneg_triple(annulus, "annulus", what)
        self.shape, self.gap, self.annulus, self.device = shape, gap, annulus, device
        self.boxes = _box_table(boxes, "boxes", what, shape)
        self.cores = _box_table(cores, "cores", what, shape)
        if len(self.cores) != len(self.boxes):
            raise ValueError(f"{what}: one core per box, got {len(self.cores)} for {len(self.boxes)}")
        b, c = self.boxes, self.cores
        if ((c[:, 0::2] < b[:, 0::2]) | (c[:, 1::2] > b[:, 1::2])).any():
            raise ValueError(f"{what}: every core lies inside its box")
        size = (b[:, 1::2] - b[:, 0::2]).astype(np.int64)
        count = size.prod(axis=1)
        if (count >= 1 << 31).any():
            raise ValueError(f"{what}: a box of 2^31 voxels or more")
        self.N = len(b)
        self.offsets = np.zeros(self.N + 1, dtype=np.int64)
        np.cumsum(count, out=self.offsets[1:])
        self.V = int(self.offsets[-1])
        self.shell_outer, self.shell_inner = np.zeros_like(b), np.zeros_like(b)
        live = count > 0
        for k in range(3):
            for table, grow in ((self.shell_outer, gap[k] + annulus[k]), (self.shell_inner, gap[k])):
                table[live, 2 * k] = np.maximum(b[live, 2 * k] - grow, 0)
                table[live, 2 * k + 1] = np.minimum(b[live, 2 * k + 1] + grow, shape[k])
        self._occupancy = None

    @property
    def occupancy(self):
        if self._occupancy is None:
            self._occupancy = roi_mark(self.boxes, self.shape, self.device)
        return self._occupancy


def footprint_geometry(boxes, cores, shape, gap=(1, 2, 2), annulus=(2, 4, 4), device="cuda"):
    """``FootprintGeometry(boxes, cores, shape, gap, annulus, device)``: the tables are checked here, on the host, once."""
    return FootprintGeometry(boxes, cores, shape, gap, annulus, device)


def _host(a):
    return C.c_void_p(a.ctypes.data)


def _volumes(x, shape, what):
    """(x, T, time stride) of a float32 device stack [T, D, H, W] with contiguous volumes of ``shape``."""
    _dev(x, "volumes")
    if x.dim() != 4 or (shape is not None and tuple(x.shape[1:]) != tuple(shape)):
        want = "D, H, W" if shape is None else ", ".join(str(s) for s in shape)
        raise ValueError(f"{what}: volumes [T', {want}] are expected, got {tuple(x.shape)}")
    T, m = x.shape[0], x[0].numel() if x.shape[0] else 0
    if T and m and (not x[0].is_contiguous() or (T > 1 and x.stride(0) < m)):
        x = x.contiguous()
    return x, T, (x.stride(0) if T > 1 else m)


def roi_mark(boxes, shape, device="cuda"):
    """uint8 [D,H,W] on ``device``: 1 inside any box of the integer [N,6] host table, 0 elsewhere."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or min(shape) < 0:
        raise ValueError(f"roi_mark: shape is (D, H, W), got {shape!r}")
    bx = _box_table(boxes, "boxes", "roi_mark", shape)
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"roi_mark: cwfa_amd runs on MI355X only -- got device {device!r} (no CPU fallback exists)")
    L = _lib.lib()
    occ = torch.empty(shape, dtype=torch.uint8, device=device)
    check(L.cwfa_roi_mark_u8(_host(bx), len(bx), _p(occ), *shape, _stream()), "roi_mark")
    return occ


def roi_weighted_sums(stack, boxes, weights=None, offsets=None):
    """float64 [N, T]: sum over box n of weights[offsets[n] + i] * stack[t, voxel i] (box-linear i), or the plain box sum for
    ``weights=None``.  ``boxes``: integer [N,6] host table inside the volume; ``weights``: float32 device [V]; ``offsets``: the int64
    [N+1] host table of ``FootprintGeometry``.  Each product is exact in float64; a fixed tree adds them."""
    import numpy as np
    stack, T, ss = _volumes(stack, None, "roi_weighted_sums")
    D, H, W = stack.shape[1:]
    bx = _box_table(boxes, "boxes", "roi_weighted_sums", (D, H, W))
    off = None
    if weights is not None:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1)) if offsets is not None else None
        if off is None or len(off) != len(bx) + 1:
            raise ValueError("roi_weighted_sums: weights need the int64 [N+1] offsets of the boxes")
        _dev(weights, "weights")
        if weights.dim() != 1 or weights.numel() != int(off[-1]) or not weights.is_contiguous():
            raise ValueError(f"roi_weighted_sums: weights is a contiguous [V] tensor, V = offsets[N] = {int(off[-1])}")
    L = _lib.lib()
    out = torch.empty(len(bx), T, dtype=torch.float64, device=stack.device)
    check(L.cwfa_roi_weighted_sums_f32(_p(stack), _host(bx), None if off is None else _host(off), _p(weights), _p(out), T, D, H, W, len(bx),
                                       ss, _stream()), "roi_weighted_sums")
    return out


def roi_shell_sums(stack, geometry):
    """(sums float64 [N,T], counts int32 [N]) of the neuropil shells of ``geometry``: outer box minus inner box minus every occupied
    voxel.  A shell without voxels has count 0 and sum 0."""
    if not isinstance(geometry, FootprintGeometry):
        raise ValueError("roi_shell_sums: geometry is a FootprintGeometry (ops.footprint_geometry)")
    stack, T, ss = _volumes(stack, geometry.shape, "roi_shell_sums")
    L = _lib.lib()
    g = geometry
    sums = torch.empty(g.N, T, dtype=torch.float64, device=stack.device)
    counts = torch.zeros(g.N, dtype=torch.int32, device=stack.device)
    check(L.cwfa_roi_shell_sums_f32(_p(stack), _host(g.shell_outer), _host(g.shell_inner), _p(g.occupancy), _p(sums), _p(counts), T,
                                    *g.shape, g.N, ss, _stream()), "roi_shell_sums")
    return sums, counts


def footprint_state(geometry, device="cuda"):
    """The state of the footprint pass for ``geometry``: (x0 float32 [V], acc float64 [4,V] = s1, s2, sc, su, ref float64 [N,7] = c0,
    u0, e1, e2, g1, g2, eg), 36 bytes per box voxel, uninitialised -- the first ``footprint_update`` (``first=True``) writes all of it."""
    if not isinstance(geometry, FootprintGeometry):
        raise ValueError("footprint_state: geometry is a FootprintGeometry (ops.footprint_geometry)")
    return (torch.empty(geometry.V, dtype=torch.float32, device=device), torch.empty(4, geometry.V, dtype=torch.float64, device=device),
            torch.empty(geometry.N, 7, dtype=torch.float64, device=device))


def _footprint(state, geometry, what):
    if not isinstance(geometry, FootprintGeometry):
        raise ValueError(f"{what}: geometry is a FootprintGeometry (ops.footprint_geometry)")
    shapes = ((geometry.V,), (4, geometry.V), (geometry.N, 7))
    if len(state) != 3 or any(not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != s
                              for t, dt, s in zip(state, (torch.float32, torch.float64, torch.float64), shapes)):
        raise ValueError(f"{what}: the state is (x0 float32 {shapes[0]}, acc float64 {shapes[1]}, ref float64 {shapes[2]}), contiguous, on "
                         f"the HIP device (ops.footprint_state)")


def _ref_trace(t, N, T, name, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64 or tuple(t.shape) != (N, T):
        raise ValueError(f"{what}: {name} is a float64 [{N}, {T}] tensor on the HIP device")
    return t if t.is_contiguous() else t.contiguous()


def footprint_update(x, geometry, c, u, state, first):
    """Add the chunk ``x`` [T',D,H,W] to ``state`` (``footprint_state``).  ``c``: float64 device [N,T'], the seed traces of the chunk;
    ``u``: the neuropil traces, or None (su, g1, g2, eg stay 0.0).  Per box voxel, d = x - x0 (x0 its first sample ever seen), e = c - c0,
    g = u - u0: s1 += d, s2 += d d, sc += d e, su += d g, and per neuron e1, e2, g1, g2, eg likewise, in float64, in time order; the
    first chunk skips its own first volume.  Any chunking gives the same bits."""
    what = "footprint_update"
    _dev(x, "x")
    _footprint(state, geometry, what)
    x, T, ss = _volumes(x, geometry.shape, what)
    if first and T < 1:
        raise ValueError(f"{what}: the first chunk needs at least one volume")
    g = geometry
    c = _ref_trace(c, g.N, T, "c", what)
    u = None if u is None else _ref_trace(u, g.N, T, "u", what)
    L = _lib.lib()
    check(L.cwfa_footprint_update_f32(_p(x), _host(g.boxes), _host(g.offsets), _p(c), _p(u), *(_p(t) for t in state), T, *g.shape, g.N, ss,
                                      int(bool(first)), _stream()), what)
    return state


def footprint_corr(state, geometry, count, neuropil=True):
    """float32 [V]: per box voxel the correlation of its series with its neuron's seed trace after ``count`` samples -- the partial
    correlation given the neuropil trace for ``neuropil=True`` -- in float64 from ``state``.  A constant series, NaN, inf and
    ``count`` = 1 give 0, never NaN.  The state is only read."""
    what = "footprint_corr"
    _footprint(state, geometry, what)
    if int(count) < 1:
        raise ValueError(f"{what}: needs at least one sample")
    L = _lib.lib()
    corr = torch.empty(geometry.V, dtype=torch.float32, device=state[0].device)
    check(L.cwfa_footprint_corr_f32(_p(state[1]), _p(state[2]), _host(geometry.offsets), geometry.N, int(count), int(bool(neuropil)),
                                    _p(corr), _stream()), what)
    return corr


def footprint_threshold(thr, what):
    thr = float(thr)
    if not 0.0 < thr <= 1.0:
        raise ValueError(f"{what}: thr = {thr} is not in (0, 1]")
    return thr


def footprint_select(corr, geometry, thr):
    """(weights float32 [V], wsum float64 [N], sizes int32 [N]): per neuron the voxels with ``corr >= thr`` (0 < thr <= 1) that are
    connected through faces, inside the box, to such a voxel of the neuron's core; weights = corr there, 0 elsewhere; wsum: their
    float64 sum in box-linear order.  Boxes hold at most 2^15 voxels."""
    what = "footprint_select"
    thr = footprint_threshold(thr, what)
    if not isinstance(geometry, FootprintGeometry):
        raise ValueError(f"{what}: geometry is a FootprintGeometry (ops.footprint_geometry)")
    g = geometry
    if g.N and int((g.offsets[1:] - g.offsets[:-1]).max()) > _lib.FOOTPRINT_SELECT_MAX:
        raise ValueError(f"{what}: a box of more than {_lib.FOOTPRINT_SELECT_MAX} voxels")
    _dev(corr, "corr")
    if corr.dim() != 1 or corr.numel() != g.V or not corr.is_contiguous():
        raise ValueError(f"{what}: corr is a contiguous [V] tensor, V = {g.V}")
    L = _lib.lib()
    w = torch.empty_like(corr)
    wsum = torch.empty(g.N, dtype=torch.float64, device=corr.device)
    sizes = torch.empty(g.N, dtype=torch.int32, device=corr.device)
    check(L.cwfa_footprint_select_f32(_p(corr), _host(g.boxes), _host(g.cores), _host(g.offsets), g.N, _f32(thr), _p(w), _p(wsum),
                                      _p(sizes), _stream()), what)
    return w, wsum, sizes


# ------------------------------------------------------------------------------------------------ demixing of overlapping footprints
def footprint_pairs(boxes):
    """int32 [P,2] on the host: every (n, m), n <= m, whose boxes (an integer [N,6] table) share a voxel, ascending in (n, m); the
    diagonal (n, n) of every box is included, empty or not.  Blocks of rows against all later boxes in numpy: no Python loop over
    pairs."""
    import numpy as np
    b = _box_table(boxes, "boxes", "footprint_pairs")
    N = len(b)
    lo, hi = b[:, 0::2], b[:, 1::2]
    if ((lo < 0) | (lo > hi)).any():
        raise ValueError("footprint_pairs: every row of boxes is a half-open range (z0, z1, y0, y1, x0, x1)")
    live = (hi > lo).all(axis=1)
    out = []
    for r0 in range(0, N, 256):
        r1 = min(N, r0 + 256)
        hit = live[r0:r1, None] & live[None, r0:]
        for k in range(3):
            hit &= (lo[r0:r1, None, k] < hi[None, r0:, k]) & (lo[None, r0:, k] < hi[r0:r1, None, k])
        rows = np.arange(r1 - r0)
        hit[rows, rows] = True                                                    # the diagonal, also of an empty box
        hit &= rows[:, None] <= np.arange(N - r0)[None, :]
        n, m = np.nonzero(hit)
        out.append(np.stack([n + r0, m + r0], axis=1))
    pairs = np.concatenate(out) if out else np.zeros((0, 2))
    return np.ascontiguousarray(pairs.astype(np.int32))


def _pair_table(pairs, N, what):
    import numpy as np
    try:
        q = np.asarray(pairs)
        ok = q.size == 0 or (np.issubdtype(q.dtype, np.integer) and q.ndim == 2 and q.shape[1] == 2)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: pairs is an integer [P,2] table (ops.footprint_pairs)")
    q = np.ascontiguousarray(q.reshape(-1, 2).astype(np.int32))
    key = q[:, 0].astype(np.int64) * max(N, 1) + q[:, 1]
    if len(q) and ((q[:, 0] < 0) | (q[:, 0] > q[:, 1]) | (q[:, 1] >= N) | (np.diff(key, prepend=-1) <= 0)).any():
        raise ValueError(f"{what}: every row of pairs is 0 <= n <= m < {N}, ascending in (n, m)")
    return q


def footprint_overlaps(footprints, pairs):
    """float64 [P] on the device: G[p] = sum over the intersection of boxes n and m of w_n(v) w_m(v) for ``pairs[p]`` = (n, m).
    ``footprints``: what ``NeuronFootprints.finish`` returns (``boxes``, ``offsets`` on the host, ``weights`` float32 [V] on the
    device); ``pairs``: ``footprint_pairs``' table.  Each product is exact in float64; one wave adds a pair's in a fixed tree."""
    import numpy as np
    what = "footprint_overlaps"
    try:
        boxes, offsets, w = footprints.boxes, footprints.offsets, footprints.weights
    except AttributeError:
        raise ValueError(f"{what}: footprints is what NeuronFootprints.finish returns") from None
    bx = _box_table(boxes, "boxes", what)
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    if len(off) != len(bx) + 1:
        raise ValueError(f"{what}: offsets is the int64 [N+1] table of the boxes")
    q = _pair_table(pairs, len(bx), what)
    _dev(w, "weights")
    if w.dim() != 1 or w.numel() != int(off[-1]) or not w.is_contiguous():
        raise ValueError(f"{what}: weights is a contiguous [V] tensor, V = offsets[N] = {int(off[-1])}")
    L = _lib.lib()
    G = torch.empty(len(q), dtype=torch.float64, device=w.device)
    ws = torch.empty(len(q) * _lib.DEMIX_PAIR_BYTES // 8, dtype=torch.int64, device=w.device)
    check(L.cwfa_footprint_overlaps_f32(_p(w), _host(bx), _host(off), len(bx), _host(q), len(q), _p(ws), _p(G), _stream()), what)
    return G


def demix_structure(pairs, N):
    """(rowptr int32 [N+1], col int32 [E]) on the host: the directed CSR pattern of ``pairs``' off-diagonal entries, (n, m) and
    (m, n) for every pair n < m, columns ascending within a row."""
    import numpy as np
    q = _pair_table(pairs, N, "demix_structure")
    off = q[q[:, 0] != q[:, 1]]
    rows, cols = np.concatenate([off[:, 0], off[:, 1]]), np.concatenate([off[:, 1], off[:, 0]])
    order = np.lexsort((cols, rows))
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=rowptr[1:])
    if rowptr[-1] >= 1 << 31:
        raise ValueError("demix_structure: 2^31 entries or more")
    return rowptr.astype(np.int32), np.ascontiguousarray(cols[order].astype(np.int32))


class DemixPlan:
    """What demixing needs of a recording's footprints, computed once: on the host ``pairs`` int32 [P,2] (``footprint_pairs``) and the
    directed CSR pattern ``rowptr`` int32 [N+1], ``col`` int32 [E]; on the device ``G`` float64 [P] (``footprint_overlaps``) and ``val``
    float64 [E], the mixing coefficients M_nm = (G_nm wsum_m) / (G_mm wsum_n) of the entries (0.0 where G_nm == 0, a denominator is
    not > 0 or a footprint is empty).  The index arrays the kernels read are the library's own checked copy, behind ``handle``."""

    def __init__(self, footprints, pairs=None):
        import numpy as np
        what = "DemixPlan"
        try:
            wsum, sizes = footprints.wsum, footprints.sizes
            N = len(footprints.boxes)
        except (AttributeError, TypeError):
            raise ValueError(f"{what}: footprints is what NeuronFootprints.finish returns") from None
        self.N = N
        self.pairs = footprint_pairs(footprints.boxes) if pairs is None else _pair_table(pairs, N, what)
        for t, dt, name in ((wsum, torch.float64, "wsum"), (sizes, torch.int32, "sizes")):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or tuple(t.shape) != (N,) or not t.is_contiguous():
                raise ValueError(f"{what}: {name} is a contiguous {dt} [{N}] tensor on the HIP device")
        self.rowptr, self.col = demix_structure(self.pairs, N)
        self.E = len(self.col)
        self.G = footprint_overlaps(footprints, self.pairs)
        self.device = self.G.device
        L = _lib.lib()
        handle = C.c_void_p()
        self.handle = None
        check(L.cwfa_demix_plan_create(_host(self.rowptr), _host(self.col), N, _host(self.pairs), len(self.pairs), C.byref(handle)), what)
        self.handle = handle
        self.val = torch.empty(self.E, dtype=torch.float64, device=self.device)
        check(L.cwfa_demix_coeffs_f64(self.handle, _p(self.G), len(self.pairs), _p(wsum), _p(sizes), N, _p(self.val), _stream()), what)

    def __del__(self):
        handle, self.handle = getattr(self, "handle", None), None
        if handle is not None:
            try:
                _lib.lib().cwfa_demix_plan_destroy(handle)
            except Exception:                                                     # interpreter shutdown
                pass


def demix_solve(F, plan, n_sweeps=64, tol=0.0, nonneg=True):
    """(Fd float64 [N,T], sweeps int32 [T]): projected Gauss-Seidel on F_n = f_n + sum_m M_nm f_m, independently per time step, from
    f = F, n = 0 .. N-1 per sweep, a row's entries by ascending m; with ``nonneg`` a negative value becomes 0.  A time step ends
    after the first sweep in which every change is <= ``tol``, or after ``n_sweeps``.  ``F``: float64 device [N,T], rows contiguous,
    any row stride; rows of empty footprints come back NaN and feed nobody."""
    what = "demix_solve"
    if not isinstance(plan, DemixPlan):
        raise ValueError(f"{what}: plan is a DemixPlan")
    n_sweeps, tol = int(n_sweeps), float(tol)
    if n_sweeps < 1:
        raise ValueError(f"{what}: n_sweeps = {n_sweeps} is not positive")
    if not tol >= 0.0:
        raise ValueError(f"{what}: tol = {tol} is negative or NaN")
    F, N, T, stride = _rows(F, what, "F")
    if N != plan.N:
        raise ValueError(f"{what}: F has {N} rows, the plan {plan.N} neurons")
    if F.device != plan.device:
        raise ValueError(f"{what}: F is on {F.device}, the plan on {plan.device}")
    L = _lib.lib()
    out = torch.empty(N, T, dtype=torch.float64, device=F.device)
    sweeps = torch.empty(T, dtype=torch.int32, device=F.device)
    check(L.cwfa_demix_solve_f64(_p(F), stride, _p(out), N, T, plan.handle, min(n_sweeps, 0x7fffffff), tol, int(bool(nonneg)), _p(sweeps),
                                 _stream()), what)
    return out, sweeps


# ------------------------------------------------------------------------------------------------ trace post-processing
def _rows(x, what, name="traces"):
    """A float64 device [N, T] tensor with contiguous rows (T >= 1) as (tensor, N, T, row stride in elements): a view with a row
    stride of at least T qualifies without a copy.  Anything else is refused, before any device work."""
    if not torch.is_tensor(x):
        raise TypeError(f"{what}: {name}: expected a torch.Tensor, got {type(x)}")
    if x.dtype != torch.float64:
        raise TypeError(f"{what}: {name}: expected float64, got {x.dtype}")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"{what}: {name} is [N, T] with T >= 1, got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: cwfa_amd runs on MI355X only -- got a {x.device} tensor (no CPU fallback exists)")
    N, T = int(x.shape[0]), int(x.shape[1])
    if N and ((T > 1 and x.stride(1) != 1) or (N > 1 and x.stride(0) < T)):
        x = x.contiguous()
    return x, N, T, (int(x.stride(0)) if N > 1 else T)


def sliding_quantile_limits():
    """(tile, max_half_lds): the outputs a workgroup of the LDS form of ``sliding_quantile`` owns, and the largest half window that
    form takes.  Host only."""
    tile, most = C.c_int(0), C.c_int(0)
    check(_lib.lib().cwfa_sliding_quantile_limits(C.byref(tile), C.byref(most)), "sliding_quantile_limits")
    return tile.value, most.value


def sliding_quantile(x, half_window, percentile, form="auto"):
    """float64 [N, T]: out[n, t] = the k-th smallest (from 0) of x[n, lo..hi], lo = max(0, t - h), hi = min(T - 1, t + h),
    k = (p * (hi - lo)) // 100 -- an element of the series, bit for bit, without interpolation; -0 and +0 are one value (returned as
    +0) and NaN sorts last.  ``x``: float64 device [N, T], rows contiguous, any row stride.  ``form``: "lds" (half windows up to
    ``sliding_quantile_limits()[1]``), "stream" (any) or "auto"."""
    what = "sliding_quantile"
    if form not in _lib.SELECT_FORM:
        raise ValueError(f"{what}: form is one of {sorted(_lib.SELECT_FORM)}, got {form!r}")
    h, p = int(half_window), int(percentile)
    if h != half_window or h < 0:
        raise ValueError(f"{what}: the half window is a non-negative integer, got {half_window!r}")
    if p != percentile or not 0 <= p <= 100:
        raise ValueError(f"{what}: the percentile is an integer in 0 .. 100, got {percentile!r}")
    x, N, T, stride = _rows(x, what, "x")
    L = _lib.lib()
    out = torch.empty(N, T, dtype=torch.float64, device=x.device)
    check(L.cwfa_sliding_quantile_f64(_p(x), N, T, stride, min(h, 0x7fffffff), p, _p(out), _lib.SELECT_FORM[form], _stream()), what)
    return out


def trace_select(x, ranks):
    """float64 [K, N]: out[k, n] = the ``ranks[k]``-th smallest (from 0) of row n of the float64 device [N, T] tensor ``x``, 1 to 4
    ranks in 0 .. T - 1, in the order of ``sliding_quantile``: the row-major float64 twin of ``temporal_select``."""
    what = "trace_select"
    ranks = [int(r) for r in ranks]
    if not 1 <= len(ranks) <= 4:
        raise ValueError(f"{what}: 1 to 4 ranks, got {len(ranks)}")
    x, N, T, stride = _rows(x, what, "x")
    if any(r < 0 or r >= T for r in ranks):
        raise ValueError(f"{what}: ranks {ranks} are not in 0 .. {T - 1}")
    L = _lib.lib()
    out = torch.empty(len(ranks), N, dtype=torch.float64, device=x.device)
    check(L.cwfa_trace_select_f64(_p(x), N, T, stride, (C.c_int * len(ranks))(*ranks), len(ranks), _p(out), _stream()), what)
    return out


def ar1_deconv(y, gamma, lam):
    """(c, s, pools): per row of the float64 device [N, T] tensor ``y`` the minimiser of 1/2 sum (y - c)^2 + lam sum s under
    s_0 = c_0 >= 0, s_t = c_t - gamma c_{t-1} >= 0, by the pool algorithm (exact).  ``gamma``: a float in [0, 1); ``lam``: float64
    device [N].  c, s: float64 [N, T]; pools: int32 [N].  A row with a non-finite sample, or a lam that is NaN, infinite or
    negative, gets NaN in c and s and 0 pools."""
    import numpy as np
    what = "ar1_deconv"
    gamma = float(gamma)
    if not 0.0 <= gamma < 1.0:
        raise ValueError(f"{what}: gamma = {gamma} is not in [0, 1)")
    y, N, T, stride = _rows(y, what, "y")
    lam = _vec(lam, N, "lam", what, torch.float64)
    L = _lib.lib()
    table = np.full(T + 1, gamma)
    table[0] = 1.0
    pw = torch.from_numpy(np.multiply.accumulate(table)).to(y.device)             # pw[k] = pw[k - 1] * gamma, rounded one by one
    c = torch.empty(N, T, dtype=torch.float64, device=y.device)
    s = torch.empty_like(c)
    pools = torch.empty(N, dtype=torch.int32, device=y.device)
    ws = torch.empty(max((int(L.cwfa_ar1_deconv_workspace_bytes(N, T)) + 7) // 8, 1), dtype=torch.float64, device=y.device)
    check(L.cwfa_ar1_deconv_f64(_p(y), N, T, stride, gamma, _p(lam), _p(pw), _p(c), _p(s), _p(pools), _p(ws), _stream()), what)
    return c, s, pools
