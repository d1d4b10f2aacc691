"""float64 restatements for the likelihood-map tests (CPU, torch): cwfa_chain_nll_map_f32, cwfa_nll_compose_f32 and the walk that
tells where the latent of a volume position starts, on the stage dicts of tests/posterior_ref.py.  The stages
are those of the INVERSE direction, in its execution order."""
import math

import torch

from posterior_ref import _gather, stage_s, stage_t

SQRT2 = math.sqrt(2.0)
POS_SHAPE, POS_SEED = (1, 3, 24, 64), 20240229          # the sampler case of tests/test_gpu_nllmap.py (checked on the CPU first)


def collapse(stages, shape):
    """(a, o, M_o, sum |s|) per volume position: the inverse chain collapsed to d = exp(-a) z + o,
        (a, o) <- gather_k(a, o);  o <- (o - t_k) exp(-s_k);  a <- a + s_k        from (0, 0)
    with M_o the same walk on absolute values (the scale the rounding errors of o are relative to) and the travelling sum of |s|."""
    a = torch.zeros(shape, dtype=torch.float64)
    o, M, sabs = a.clone(), a.clone(), a.clone()
    for st in stages:
        a, o, M, sabs = (_gather(v, st) for v in (a, o, M, sabs))
        s, t = stage_s(st), stage_t(st)
        if t is not None:
            o = o - t
            M = M + t.abs()
        if s is not None:
            o = o * torch.exp(-s)
            M = M * torch.exp(-s)
            a = a + s
            sabs = sabs + s.abs()
    return a, o, M, sabs


def chain_nll_map(x, stages):
    """dict of float64 tensors [B,C,H,W]: low, d, a, o, z = (d - o) exp(a), nll = z^2 / 2 - a, M = (|d| + M_o) exp(a) (the scale of
    z's rounding errors), sabs = sum of |s| along the path, and nll_sum [B]."""
    x = x.double()
    low, d = (x[:, 0::2] + x[:, 1::2]) / SQRT2, (x[:, 0::2] - x[:, 1::2]) / SQRT2
    a, o, Mo, sabs = collapse(stages, tuple(d.shape))
    z = (d - o) * torch.exp(a)
    nll = 0.5 * z * z - a
    return {"low": low, "d": d, "a": a, "o": o, "z": z, "nll": nll, "M": (d.abs() + Mo) * torch.exp(a), "sabs": sabs,
            "nll_sum": nll.flatten(1).sum(1)}


def start_positions(stages, shape):
    """int64 [C,H,W]: the linear index (within one sample) at which the latent that ARRIVES at each volume position STARTS -- an
    index tensor walked through the gathers of the inverse chain.  chain_fwd's z (laid out where the latents start) is read
    through it: z_map = z_fwd.flatten(1)[:, start_positions]."""
    C, H, W = shape[-3:]
    idx = torch.arange(C * H * W).view(1, C, H, W)
    for st in stages:
        idx = _gather(idx, st)
    return idx[0]


def at_positions(v, stages):
    """a [B,C,H,W] tensor laid out where the latents start, re-laid to the volume positions they arrive at"""
    idx = start_positions(stages, tuple(v.shape))
    return v.flatten(1)[:, idx.flatten()].view(v.shape)


def compose(levels, dtype=torch.float64):
    """out[b,d] = sum_n 2^-(n+1) level_n[b, d >> (n+1)], added finest first in ``dtype`` (fp32: the kernel's own expression -- every
    product is exact, so it is reproduced bit for bit)."""
    out = None
    for n, lv in enumerate(levels):
        term = lv.to(dtype).repeat_interleave(2 ** (n + 1), dim=1) * (0.5 ** (n + 1))
        out = term if out is None else out + term
    return out


def random_stages(shape, axes, seed, no_s=(), no_t=(), kinds=None, pres=None, clamps=None):
    """seeded stage dicts on the CPU (the draws of test_gpu_posterior.make_chain, without a device)"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, ax in enumerate(axes):
        s_raw = None if k in no_s else torch.randn(shape, generator=g)
        t = None if k in no_t else torch.randn(shape, generator=g)
        perm = None if ax is None else torch.randperm([0, C, H, W][ax], generator=g)
        out.append({"s_raw": s_raw, "t": t, "perm": perm, "axis": ax, "kind": kinds[k] if kinds else "ATAN",
                    "clamp": clamps[k] if clamps else 2.0, "pre": pres[k] if pres else 1.0, "neg": k == len(axes) - 1})
    return out
