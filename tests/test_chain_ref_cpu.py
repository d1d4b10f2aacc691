"""CPU: the float64 restatements of tests/chain_ref.py checked on their own -- round trips, a per-position loop that walks the
gathers backwards as chain_fwd_kernel / chain_inv_kernel do (a second statement of the index algebra, with scalar math for the clamps),
and the restatement the backward test already uses."""
import math

import pytest
import torch

import chain_ref as R


def make_stages(shape, axes, seed, kinds=None, no_s=(), no_t=(), pres=None, neg_last=True):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    kinds = kinds or ["ATAN", "TANH", "SIGMOID", "NONE"]
    out = []
    for k, ax in enumerate(axes):
        kind = kinds[k % len(kinds)]
        out.append({"s_raw": None if k in no_s else torch.randn(shape, generator=g, dtype=torch.float64),
                    "t": None if k in no_t else torch.randn(shape, generator=g, dtype=torch.float64),
                    "perm": None if ax is None else torch.randperm([0, C, H, W][ax], generator=g), "axis": ax,
                    "kind": kind, "clamp": 0.5 if kind == "NONE" else 1.5, "pre": pres[k] if pres else 1.0,
                    "neg": neg_last and k == len(axes) - 1})
    return out


CHAINS = {1: [3], 6: [None, 3, 1, 2, 3, 1], 8: [3, 1, 3, 2, None, 3, 1, 2]}


@pytest.mark.parametrize("n", [1, 6, 8])
@pytest.mark.parametrize("with_final", [False, True])
def test_inverse_undoes_forward(n, with_final):
    shape = (2, 3, 4, 5)
    g = torch.Generator().manual_seed(n)
    x = torch.randn(2, 6, 4, 5, generator=g, dtype=torch.float64)
    for axes in ([1], [2], [3]) if n == 1 else (CHAINS[n],):
        assert n == 1 or {1, 2, 3} <= set(axes)
        stages = make_stages(shape, axes, 10 * n + len(axes), no_s=(2,), no_t=(1,), pres=[1.0, 0.1] * 4)
        fp = torch.randperm(3, generator=g) if with_final else None
        z, low, ld, sumsq = R.chain_fwd(x, stages, fp)
        back, ld_inv = R.chain_inv(z, low, R.inverse_stages(stages, fp))
        assert float((back - x).abs().max()) <= 1e-12 * float(x.abs().max())
        assert float((ld + ld_inv).abs().max()) <= 1e-12 * float(R.sum_abs_s(stages, low).max())
        assert abs(sumsq - float((z ** 2).sum())) <= 1e-12 * sumsq
        if any(st["s_raw"] is not None for st in stages):
            assert float(ld.abs().min()) > 0


def _scalar_clamp(a, kind, clamp):
    if kind == "ATAN":
        return clamp * 0.636 * math.atan(a)
    if kind == "TANH":
        return clamp * math.tanh(a)
    if kind == "SIGMOID":
        return clamp * 2.0 * (1.0 / (1.0 + math.exp(-a)) - 0.5)
    return clamp * a


def _scalar_st(st, b, p):
    c, h, w = p
    s = 0.0 if st["s_raw"] is None else _scalar_clamp(float(st["s_raw"][b, c, h, w]) * st["pre"], st["kind"], st["clamp"])
    t = 0.0
    if st["t"] is not None:
        tv = float(st["t"][b, c, h, w])
        t = -tv / math.sqrt(2.0) if st["neg"] else tv * st["pre"]
    return s, t


def _pull(p, st):
    """gather_pos of csrc/elementwise.hip"""
    if st["perm"] is None:
        return p
    p = list(p)
    p[st["axis"] - 1] = int(st["perm"][p[st["axis"] - 1]])
    return tuple(p)


def _walk_back(p, stages):
    where = [None] * len(stages)
    for k in range(len(stages) - 1, -1, -1):
        where[k] = p
        p = _pull(p, stages[k])
    return where, p


@pytest.mark.parametrize("n", [1, 6, 8])
def test_against_the_per_position_loop(n):
    B, C, H, W = shape = (2, 3, 4, 5)
    g = torch.Generator().manual_seed(40 + n)
    stages = make_stages(shape, CHAINS[n], 50 + n, no_s=(3,), no_t=(4,), pres=[0.1, 1.0] * 4)
    x = torch.randn(B, 2 * C, H, W, generator=g, dtype=torch.float64)
    zin = torch.randn(shape, generator=g, dtype=torch.float64)
    lowin = torch.randn(shape, generator=g, dtype=torch.float64)
    fp = torch.randperm(C, generator=g)
    z = torch.empty(shape, dtype=torch.float64)
    low = torch.empty(shape, dtype=torch.float64)
    xout = torch.empty(B, 2 * C, H, W, dtype=torch.float64)
    Mz, Mx = torch.empty_like(z), torch.empty_like(xout)
    ld_f, ld_i = [0.0] * B, [0.0] * B
    r2 = math.sqrt(2.0)
    for b in range(B):
        for c in range(C):
            for h in range(H):
                for w in range(W):
                    # forward, as chain_fwd_kernel
                    low[b, c, h, w] = (x[b, 2 * c, h, w] + x[b, 2 * c + 1, h, w]) / r2
                    where, (c0, h0, w0) = _walk_back((int(fp[c]), h, w), stages)
                    v = float(x[b, 2 * c0, h0, w0] - x[b, 2 * c0 + 1, h0, w0]) / r2
                    m = abs(v)
                    for st, p in zip(stages, where):
                        s, t = _scalar_st(st, b, p)
                        v, m = math.exp(s) * v + t, math.exp(s) * m + abs(t)
                        ld_f[b] += s
                    z[b, c, h, w], Mz[b, c, h, w] = v, m
                    # inverse, as chain_inv_kernel
                    where, (c0, h0, w0) = _walk_back((c, h, w), stages)
                    v = float(zin[b, c0, h0, w0])
                    m = abs(v)
                    for st, p in zip(stages, where):
                        s, t = _scalar_st(st, b, p)
                        v, m = (v - t) * math.exp(-s), (m + abs(t)) * math.exp(-s)
                        ld_i[b] -= s
                    lo = float(lowin[b, c, h, w])
                    xout[b, 2 * c, h, w], xout[b, 2 * c + 1, h, w] = (lo + v) / r2, (lo - v) / r2
                    Mx[b, 2 * c, h, w] = Mx[b, 2 * c + 1, h, w] = (abs(lo) + m) / r2
    rz, rlow, rld, rsq = R.chain_fwd(x, stages, fp)
    rx, rldi = R.chain_inv(zin, lowin, stages)
    tol = 1e-13
    for what, got, ref in (("z", z, rz), ("low", low, rlow), ("x", xout, rx), ("M fwd", Mz, R.chain_magnitude(stages, x=x, final_perm=fp)),
                           ("M inv", Mx, R.chain_magnitude(stages, z=zin, low=lowin, inverse=True)),
                           ("logdet fwd", torch.tensor(ld_f, dtype=torch.float64), rld), ("logdet inv", torch.tensor(ld_i, dtype=torch.float64), rldi)):
        assert float((got - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max())), what
    assert abs(rsq - float((z ** 2).sum())) <= 1e-12 * rsq
    # z = None is the walk from zeros; the magnitudes dominate the values
    x0, _ = R.chain_inv(None, lowin, stages)
    assert torch.equal(x0, R.chain_inv(torch.zeros(shape), lowin, stages)[0])
    assert bool((rz.abs() <= Mz * (1 + 1e-12)).all()) and bool((rx.abs() <= Mx * (1 + 1e-12)).all())


def test_forward_agrees_with_the_backward_tests_restatement():
    """the five-stage chain of test_chain_backward_vs_autograd through its _torch_chain"""
    from test_gpu_backward import _torch_chain
    B, Cc, H, W = shape = (2, 6, 9, 12)
    g0 = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, 2 * Cc, H, W, generator=g0).double()
    stages = []
    for k, ax in enumerate([None, 1, 2, 3, 1]):
        s_raw = torch.randn(shape, generator=g0).double()
        t = torch.randn(shape, generator=g0).double()
        perm = None if ax is None else torch.randperm([0, Cc, H, W][ax], generator=g0)
        stages.append({"s_raw": s_raw, "t": t, "perm": perm, "axis": ax, "clamp": 2.0, "pre": 1.0, "neg": k == 0})
    fp = torch.randperm(Cc, generator=g0)
    z, low, ld, _ = R.chain_fwd(x, stages, fp)
    hi = (x[:, 0::2] - x[:, 1::2]) / math.sqrt(2.0)
    zr, ldr = _torch_chain(hi, stages, fp)
    assert float((z - zr).abs().max()) <= 1e-13 * float(zr.abs().max())
    assert float((ld - ldr).abs().max()) <= 1e-12 * float(ldr.abs().max())
    assert torch.equal(low, (x[:, 0::2] + x[:, 1::2]) / math.sqrt(2.0))


def test_affine_and_channel_affine_restatements():
    shape = (2, 3, 5, 7)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    for ax in (1, 2, 3):
        st = make_stages(shape, [ax], 60 + ax, neg_last=False)[0]
        y, ld = R.affine(x, st, 0)
        # the one-stage chain on the detail band is the same map
        s, t = R.stage_s(st), R.stage_t(st)
        assert torch.equal(y, torch.exp(s) * x.index_select(ax, st["perm"]) + t)
        inv = R.inverse_stages([st])[0]
        back, ld_inv = R.affine(y, inv, 1)
        assert float((back - x).abs().max()) <= 1e-12 and float((ld + ld_inv).abs().max()) <= 1e-12
        gin = dict(st, gin=True)
        yg, ldg = R.affine(x, gin, 0)
        assert float(ldg.abs().max()) <= 1e-12                  # the channel mean is removed at every pixel
        sg = torch.log((yg - t) / x.index_select(ax, st["perm"]))
        assert float(sg.mean(1).abs().max()) <= 1e-12 and float((sg - (s - s.mean(1, keepdim=True))).abs().max()) <= 1e-12
    y0, _ = R.affine(None, st, 0, shape=shape)
    assert torch.equal(y0, R.stage_t(st))
    # channel affine: mode 1 with the inverse permutation undoes mode 0
    sc, sh = torch.rand(3, generator=g, dtype=torch.float64) + 0.5, torch.randn(3, generator=g, dtype=torch.float64)
    p = torch.tensor([2, 0, 1])
    q = R.inverse_perm(p)
    y = R.channel_affine(x, sc, sh, False, perm_out=p)                     # y[c] = x[p[c]] * sc[p[c]] + sh[p[c]]
    for c in range(3):
        assert torch.equal(y[:, c], x[:, p[c]] * sc[p[c]] + sh[p[c]])
    back = R.channel_affine(y, sc, sh, True, perm_in=q)                    # back[c] = (y[q[c]] - sh[c]) / sc[c]
    assert float((back - x).abs().max()) <= 1e-12
    assert torch.equal(R.channel_affine(x, None, None), x)
