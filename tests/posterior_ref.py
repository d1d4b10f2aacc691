"""float64 restatements for the posterior tests (CPU, torch): the inverse chain of cwfa_chain_inv_f32, the variance recursion of
cwfa_chain_inv_var_f32 with the four clamp kinds of csrc/common.h, and the variance of the truncated standard normal.

A stage is a dict: ``s_raw`` / ``t`` ([B,C,H,W] or None), ``perm`` (index table or None) with ``axis`` (1 / 2 / 3), ``kind``
('NONE' | 'ATAN' | 'TANH' | 'SIGMOID', default 'ATAN'), ``clamp`` (default 2.0), ``pre`` (pre_scale, default 1.0), ``neg``
(t := -t / sqrt 2, default False); ``s`` may hold an already clamped coefficient instead of ``s_raw``.  Stages are in the execution
order of the inverse."""
import math

import numpy as np
import torch


def soft_clamp(a, kind, clamp):
    """cwfa_soft_clamp (csrc/common.h)."""
    if kind == "ATAN":
        return clamp * (0.636 * torch.atan(a))
    if kind == "TANH":
        return clamp * torch.tanh(a)
    if kind == "SIGMOID":
        return clamp * (2.0 * (torch.sigmoid(a) - 0.5))
    if kind == "NONE":
        return clamp * a
    raise ValueError(kind)


def stage_s(st):
    if st.get("s") is not None:
        return st["s"].double()
    if st.get("s_raw") is None:
        return None
    return soft_clamp(st["s_raw"].double() * st.get("pre", 1.0), st.get("kind", "ATAN"), st.get("clamp", 2.0))


def stage_t(st):
    if st.get("t") is None:
        return None
    t = st["t"].double()
    return -t / math.sqrt(2.0) if st.get("neg", False) else t * st.get("pre", 1.0)


def _gather(v, st):
    if st.get("perm") is None:
        return v
    return v.index_select(st["axis"], st["perm"].to(torch.long))


def chain_inv(z, low, stages):
    """x[B,2C,H,W] = Haar1D^-1(cat[low, v]),  v <- (gather_k(v) - t_k) * exp(-s_k) from v = z (None = zeros)."""
    low = low.double()
    v = torch.zeros_like(low) if z is None else z.double()
    for st in stages:
        v = _gather(v, st)
        s, t = stage_s(st), stage_t(st)
        if t is not None:
            v = v - t
        if s is not None:
            v = v * torch.exp(-s)
    x = torch.empty(low.shape[0], 2 * low.shape[1], *low.shape[2:], dtype=torch.float64)
    x[:, 0::2] = (low + v) / math.sqrt(2.0)
    x[:, 1::2] = (low - v) / math.sqrt(2.0)
    return x


def chain_inv_var(var_low, stages, z_var, shape=None):
    """a <- gather_k(a) - 2 s_k from a = 0;  var_v = z_var * exp(a);  out[2c] = out[2c+1] = (var_low[c] + var_v[c]) / 2."""
    if var_low is not None:
        shape = tuple(var_low.shape)
    a = torch.zeros(shape, dtype=torch.float64)
    for st in stages:
        a = _gather(a, st)
        s = stage_s(st)
        if s is not None:
            a = a - 2.0 * s
    var = z_var * torch.exp(a)
    if var_low is not None:
        var = var + var_low.double()
    return (0.5 * var).repeat_interleave(2, dim=1)


def z_var(T, nodes=200):
    """Variance of a standard normal truncated to [-T, T] by Gauss-Legendre quadrature of z^2 phi(z) and phi(z) over [0, T]
    (both integrands positive: nothing cancels, at any T; beyond T = 40 the tails are below 1e-300)."""
    T = float(T)
    if T == 0.0:
        return 0.0
    if T > 40.0:
        return 1.0
    x, w = np.polynomial.legendre.leggauss(nodes)
    # panels of width <= 1 keep the 200-node rule far inside its convergence range for every T
    edges = np.linspace(0.0, T, max(1, int(math.ceil(T))) + 1)
    num = den = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        z = 0.5 * (hi - lo) * x + 0.5 * (hi + lo)
        phi = np.exp(-0.5 * z * z)
        num += 0.5 * (hi - lo) * float(np.sum(w * z * z * phi))
        den += 0.5 * (hi - lo) * float(np.sum(w * phi))
    return num / den


def per_element_rel(got, ref):
    """max over the elements of |got - ref| / |ref| (ref must not hold a zero)."""
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    return float(((got - ref).abs() / ref.abs()).max())
