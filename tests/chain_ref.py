"""float64 restatements for the chain and affine tests (CPU, torch): cwfa_chain_fwd_f32 / cwfa_chain_inv_f32 with their log-det and
sumsq, the magnitude walk that rounding errors are relative to, cwfa_affine_f32 (plain and GIN) and cwfa_channel_affine_f32.

Stages are the dicts of tests/posterior_ref.py (``s_raw`` / ``t`` / ``perm`` + ``axis`` / ``kind`` / ``clamp`` / ``pre`` / ``neg``), in
the execution order of the direction they are handed to."""
import math

import torch

from posterior_ref import _gather, soft_clamp, stage_s, stage_t          # noqa: F401  (soft_clamp: re-exported for the tests)
from posterior_ref import chain_inv as _chain_inv_values

SQRT2 = math.sqrt(2.0)


def _sum_s(stages, like):
    """sum of the clamped s over the stages and positions, per sample, and the same of |s|"""
    tot = torch.zeros(like.shape[0], dtype=torch.float64)
    tot_abs = torch.zeros(like.shape[0], dtype=torch.float64)
    for st in stages:
        s = stage_s(st)
        if s is not None:
            tot = tot + s.flatten(1).sum(1)
            tot_abs = tot_abs + s.abs().flatten(1).sum(1)
    return tot, tot_abs


def sum_abs_s(stages, like):
    return _sum_s(stages, like)[1]


def haar_split(x):
    x = x.double()
    return (x[:, 0::2] + x[:, 1::2]) / SQRT2, (x[:, 0::2] - x[:, 1::2]) / SQRT2


def chain_fwd(x, stages, final_perm=None):
    """(z, low, logdet[B], sumsq): low = (x[2c] + x[2c+1]) / sqrt 2, v = (x[2c] - x[2c+1]) / sqrt 2, per stage
    v <- exp(s) * gather(v) + t, z = v gathered along the channels by final_perm; logdet = sum of s, sumsq = sum of z^2."""
    low, v = haar_split(x)
    for st in stages:
        v = _gather(v, st)
        s, t = stage_s(st), stage_t(st)
        if s is not None:
            v = torch.exp(s) * v
        if t is not None:
            v = v + t
    z = v if final_perm is None else v.index_select(1, final_perm.to(torch.long))
    return z, low, _sum_s(stages, low)[0], float((z * z).sum())


def chain_inv(z, low, stages):
    """(x, logdet[B]): posterior_ref.chain_inv and logdet = -sum of s."""
    return _chain_inv_values(z, low, stages), -_sum_s(stages, low)[0]


def chain_magnitude(stages, x=None, final_perm=None, z=None, low=None, inverse=False):
    """The walks of chain_fwd / chain_inv on absolute values: the per-element scale the rounding errors of the kernels are relative to
    (exp(s) * v + t cancels, so the error of an element is not small against the element itself).
    forward (x, final_perm): M <- exp(s) * gather(M) + |t| from M = |v0|, gathered by final_perm: the scale of z.
    inverse (z or None, low): M <- (gather(M) + |t|) * exp(-s) from M = |z|; returns (|low| + M) / sqrt 2 for both outputs of a pair."""
    if not inverse:
        M = haar_split(x)[1].abs()
        for st in stages:
            M = _gather(M, st)
            s, t = stage_s(st), stage_t(st)
            if s is not None:
                M = torch.exp(s) * M
            if t is not None:
                M = M + t.abs()
        return M if final_perm is None else M.index_select(1, final_perm.to(torch.long))
    low = low.double()
    M = torch.zeros_like(low) if z is None else z.double().abs()
    for st in stages:
        M = _gather(M, st)
        s, t = stage_s(st), stage_t(st)
        if t is not None:
            M = M + t.abs()
        if s is not None:
            M = M * torch.exp(-s)
    return ((low.abs() + M) / SQRT2).repeat_interleave(2, dim=1)


def inverse_perm(perm):
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel(), dtype=perm.dtype)
    return inv


def inverse_stages(stages, final_perm=None):
    """The stages of chain_inv that undo chain_fwd(x, stages, final_perm): the forward's reversed, every gather replaced by its
    inverse and the coefficients moved with it -- v1[i] = exp(s[i]) v0[p[i]] + t[i] gives v0[j] = (v1[q[j]] - t[q[j]]) exp(-s[q[j]])
    with q the inverse of p.  final_perm becomes a leading stage that only gathers."""
    out = []
    if final_perm is not None:
        out.append({"s_raw": None, "t": None, "perm": inverse_perm(final_perm), "axis": 1})
    for st in reversed(stages):
        inv = dict(st)
        if st.get("perm") is not None:
            q = inverse_perm(st["perm"])
            inv["perm"] = q
            for key in ("s_raw", "t", "s"):
                if st.get(key) is not None:
                    inv[key] = st[key].index_select(st["axis"], q.to(torch.long)).contiguous()
        out.append(inv)
    return out


def affine(x, st, rev, shape=None):
    """(y, logdet[B]) of one stage (cwfa_affine_f32): y = exp(s) * gather(x) + t, or (gather(x) - t) * exp(-s) for rev, with
    logdet = +-sum of s.  x = None stands for zeros of ``shape``.  A GIN stage (``gin``) removes the channel mean of the clamped s at
    every pixel before use (its log-det is zero)."""
    v = torch.zeros(shape, dtype=torch.float64) if x is None else _gather(x.double(), st)
    s, t = stage_s(st), stage_t(st)
    if st.get("gin", False):
        s = s - s.mean(dim=1, keepdim=True)
    zero = torch.zeros_like(v)
    s = zero if s is None else s
    t = zero if t is None else t
    y = (v - t) * torch.exp(-s) if rev else torch.exp(s) * v + t
    ld = s.flatten(1).sum(1)
    return y, (-ld if rev else ld)


def affine_magnitude(x, st, rev, shape=None):
    """the scale of affine()'s rounding errors: exp(s) |gather(x)| + |t|, or (|gather(x)| + |t|) exp(-s)"""
    v = torch.zeros(shape, dtype=torch.float64) if x is None else _gather(x.double().abs(), st)
    s, t = stage_s(st), stage_t(st)
    if st.get("gin", False):
        s = s - s.mean(dim=1, keepdim=True)
    zero = torch.zeros_like(v)
    s = zero if s is None else s
    t = zero if t is None else t.abs()
    return (v + t) * torch.exp(-s) if rev else torch.exp(s) * v + t


def channel_affine(x, scale, shift, inverse=False, perm_in=None, perm_out=None):
    """cwfa_channel_affine_f32: output channel c takes the parameters of channel cp = perm_out[c] (c without perm_out) and reads input
    channel perm_in[c] if perm_in is given, else cp; y = x * scale + shift, or (x - shift) / scale for inverse."""
    x = x.double()
    C = x.shape[1]
    cp = torch.arange(C) if perm_out is None else perm_out.to(torch.long)
    cr = cp if perm_in is None else perm_in.to(torch.long)
    sc = torch.ones(C, dtype=torch.float64) if scale is None else scale.double()
    sh = torch.zeros(C, dtype=torch.float64) if shift is None else shift.double()
    v = x.index_select(1, cr)
    sc, sh = sc[cp].view(1, C, 1, 1), sh[cp].view(1, C, 1, 1)
    return (v - sh) / sc if inverse else v * sc + sh
