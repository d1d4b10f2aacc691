"""GPU (MI355X): the posterior of a CAT pyramid -- cwfa_chain_inv_var_f32 in both of its forms against the
float64 restatement (tests/posterior_ref.py) on the same fp32 inputs, the plan's inverse_stages, posterior_moments and
posterior_samples against inverse_pass and by-hand loops, and the reference fixture g24_posterior.

The variance spans decades, so the measure is the PER-ELEMENT relative error (posterior_ref.per_element_rel), not the max-normalised
one of conftest.rel_err.  Bounds: 4 x the worst value measured over all hand-built cases below (VAR_*), and 4 x the worst value of
the fixture / pyramid cases, which add the sub-networks' arithmetic (FIX_*); the margin covers other atanf / expf code paths of
another compiler release.  A wrong gather, a missing stage, exp(-s) for exp(-2s) or a missing 1/2 are O(1) errors."""
import math

import numpy as np
import pytest
import torch

from conftest import assert_close, load_golden, sd_of

import posterior_ref as R

pytestmark = pytest.mark.gpu

VAR_MEASURED = 1.64e-6       # worst per-element relative error over the hand-built cases, measured once on an MI355X
VAR_BOUND = 4 * VAR_MEASURED
FIX_MEASURED = 1.82e-6       # the same against the reference fixture (1.81e-6) and the by-hand pyramid (6.1e-7), measured in the same run
FIX_BOUND = 4 * FIX_MEASURED
assert VAR_BOUND < 1e-4 and FIX_BOUND < 1e-3
TOL = 1e-4                   # the golden step tests' bound (tests/test_gpu_parity.py) for the mean volume


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


def _close(what, got, ref, bound):
    err = R.per_element_rel(got, ref)
    print(f"[posterior] {what}: per-element relative error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: per-element relative error {err:.3e} > {bound:.3e}"
    return err


def _pairs_equal(out):
    return torch.equal(out[:, 0::2], out[:, 1::2])


def make_chain(shape, axes, seed, no_s=(), no_t=(), kinds=None, pres=None, clamps=None):
    """(reference stage dicts on the CPU, ops.stage list on the device, perms per stage for chain_tables) from seeded fp32 draws."""
    from cwfa_amd import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    ref, dev, perms = [], [], []
    for k, ax in enumerate(axes):
        s_raw = None if k in no_s else torch.randn(shape, generator=g)
        t = None if k in no_t else torch.randn(shape, generator=g)
        perm = None if ax is None else torch.randperm([0, C, H, W][ax], generator=g)
        kind = kinds[k] if kinds else "ATAN"
        pre = pres[k] if pres else 1.0
        clamp = clamps[k] if clamps else 2.0
        neg = k == len(axes) - 1
        ref.append({"s_raw": s_raw, "t": t, "perm": perm, "axis": ax, "kind": kind, "clamp": clamp, "pre": pre, "neg": neg})
        pd = None if perm is None else perm.cuda()
        dev.append(ops.stage(None if s_raw is None else s_raw.cuda(), None if t is None else t.cuda(), kind, clamp, pre_scale=pre,
                             t_neg_div_sqrt2=neg, perm=pd, axis=ax or 1))
        perms.append((pd, ax or 1))
    return ref, dev, perms


def _var_low(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 0.5 + 0.01


Z1 = 0.29112509477279314     # z_var(T = 1)


# ------------------------------------------------------------------------------------------------ the kernel's two forms
@pytest.mark.parametrize("shape,axes", [((2, 3, 5, 7), [3, 1, None, 2, 3, 1]), ((1, 6, 9, 12), [None, 1, 2, 3, 1])])
@pytest.mark.parametrize("with_low", [False, True])
def test_general_form(shape, axes, with_low):
    """Odd sizes and W < 64: the pull kernel."""
    from cwfa_amd import ops
    ref, dev, _ = make_chain(shape, axes, sum(shape))
    vl = _var_low(shape, 5) if with_low else None
    got = ops.chain_inv_var(None if vl is None else vl.cuda(), dev, Z1, shape=shape)
    assert got.shape == (shape[0], 2 * shape[1]) + shape[2:] and _pairs_equal(got)
    _close(f"general {shape} low={with_low}", got, R.chain_inv_var(vl, ref, Z1, shape), VAR_BOUND)


def test_rows4_form_with_and_without_tables():
    """(2, 3, 24, 64): 16 rows per block, so the second block is half dead; six stages with TWO column gathers (both exchange
    buffers), a channel gather and a row gather; composed tables or the dependent walk: bitwise the same."""
    from cwfa_amd import ops
    shape = (2, 3, 24, 64)
    ref, dev, perms = make_chain(shape, [None, 3, 1, 2, 3, 1], 77)
    vl = _var_low(shape, 6)
    tabs = ops.chain_tables(perms, None, *shape[1:], "cuda")
    for low in (None, vl):
        a = ops.chain_inv_var(None if low is None else low.cuda(), dev, Z1, shape=shape)
        b = ops.chain_inv_var(None if low is None else low.cuda(), dev, Z1, shape=shape, tables=tabs)
        assert torch.equal(a, b) and _pairs_equal(a)
        _close(f"rows4 {shape} low={low is not None}", a, R.chain_inv_var(low, ref, Z1, shape), VAR_BOUND)


def test_more_than_six_stages():
    from cwfa_amd import ops
    shape = (1, 3, 16, 64)
    ref, dev, perms = make_chain(shape, [3, 1, None, 2, 3, 1, 2], 78)
    got = ops.chain_inv_var(None, dev, Z1, shape=shape)
    assert _pairs_equal(got)
    _close("seven stages", got, R.chain_inv_var(None, ref, Z1, shape), VAR_BOUND)
    assert torch.equal(got, ops.chain_inv_var(None, dev, Z1, shape=shape, tables=ops.chain_tables(perms, None, *shape[1:], "cuda")))


def test_general_against_rows4_form():
    """The same chain on a var_low view shifted by one element (not 16-byte aligned) falls to the general form."""
    from cwfa_amd import ops
    shape = (1, 3, 16, 64)
    n = math.prod(shape)
    ref, dev, _ = make_chain(shape, [None, 3, 1, 2, 3, 1], 79)
    vl = _var_low(shape, 7)
    buf = torch.empty(n + 4, device="cuda")
    shifted = buf[1:n + 1].view(shape)
    shifted.copy_(vl)
    assert shifted.data_ptr() % 16 == 4
    aligned = ops.chain_inv_var(vl.cuda(), dev, Z1)
    general = ops.chain_inv_var(shifted, dev, Z1)
    want = R.chain_inv_var(vl, ref, Z1)
    _close("aligned run", aligned, want, VAR_BOUND)
    _close("shifted run (general form)", general, want, VAR_BOUND)
    _close("general vs 16-byte form", general, aligned, VAR_BOUND)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 16, 64)])
def test_stage_kinds(shape):
    """All four clamp kinds, pre_scale = 0.1, an s-less and a t-less stage, in both forms; the shifts never enter."""
    from cwfa_amd import ops
    kinds = ["NONE", "ATAN", "TANH", "SIGMOID", "ATAN", "TANH"]
    kw = dict(no_s=(4,), no_t=(1,), kinds=kinds, pres=[1.0, 1.0, 0.1, 1.0, 1.0, 1.0], clamps=[0.5, 2.0, 2.0, 1.5, 2.0, 1.0])
    ref, dev, _ = make_chain(shape, [3, 1, 2, None, 3, 1], 80, **kw)
    vl = _var_low(shape, 8)
    got = ops.chain_inv_var(vl.cuda(), dev, 0.7)
    assert _pairs_equal(got)
    _close(f"stage kinds {shape}", got, R.chain_inv_var(vl, ref, 0.7), VAR_BOUND)
    # other shifts everywhere (and none at all): bitwise the same output
    g = torch.Generator().manual_seed(81)
    other, none = [], []
    for r in ref:
        pd = None if r["perm"] is None else r["perm"].cuda()
        s = None if r["s_raw"] is None else r["s_raw"].cuda()
        common = dict(pre_scale=r["pre"], perm=pd, axis=r["axis"] or 1)
        other.append(ops.stage(s, (5.0 * torch.randn(shape, generator=g)).cuda(), r["kind"], r["clamp"], t_neg_div_sqrt2=not r["neg"], **common))
        none.append(ops.stage(s, None, r["kind"], r["clamp"], **common))
    assert torch.equal(ops.chain_inv_var(vl.cuda(), other, 0.7), got)
    assert torch.equal(ops.chain_inv_var(vl.cuda(), none, 0.7), got)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 24, 64)])
def test_exact_cases(shape):
    from cwfa_amd import ops
    ref, dev, _ = make_chain(shape, [3, 1, None, 2, 3, 1], 82)
    vl = _var_low(shape, 9).cuda()
    # z_var == 0: the low band's variance, halved
    out = ops.chain_inv_var(vl, dev, 0.0)
    assert torch.equal(out, (vl * 0.5).repeat_interleave(2, dim=1))
    # no s anywhere and no var_low: z_var / 2 everywhere
    _, plain, _ = make_chain(shape, [3, 1, None, 2, 3, 1], 82, no_s=range(6))
    out = ops.chain_inv_var(None, plain, Z1, shape=shape)
    assert torch.equal(out, torch.full_like(out, float(np.float32(Z1) * np.float32(0.5))))
    # gathers alone (no tensors in any stage) and an empty chain
    gathers = [ops.stage(None, None, perm=torch.randperm(shape[3]).cuda(), axis=3), ops.stage(None, None)]
    for stages in (gathers, []):
        out = ops.chain_inv_var(None, stages, 0.25, shape=shape)
        assert out.is_cuda and torch.equal(out, torch.full_like(out, 0.125))
    # the two planes of a pair are identical
    assert _pairs_equal(ops.chain_inv_var(vl, dev, Z1))


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 24, 64)])
def test_std_scale(shape):
    """std_scale = 3.5 against 3.5 * sqrt(v) in float64 of the separately launched fp32 variance v: one sqrt, one product and
    std_scale rounded to fp32 -> per-element relative error <= 4 * 2^-24."""
    from cwfa_amd import ops
    ref, dev, _ = make_chain(shape, [3, 1, None, 2, 3, 1], 83)
    vl = _var_low(shape, 10).cuda()
    v = ops.chain_inv_var(vl, dev, Z1)
    std = ops.chain_inv_var(vl, dev, Z1, std_scale=3.5)
    _close(f"std_scale {shape}", std, 3.5 * v.double().sqrt(), 4 * 2.0 ** -24)
    assert _pairs_equal(std)


def test_errors():
    from cwfa_amd import ops
    from cwfa_amd._lib import CwfaHipError
    shape = (1, 2, 4, 8)
    _, dev, _ = make_chain(shape, [3, 1], 84)
    with pytest.raises(CwfaHipError):
        ops.chain_inv_var(None, dev, -0.1, shape=shape)
    with pytest.raises(CwfaHipError):
        ops.chain_inv_var(None, dev, float("nan"), shape=shape)
    with pytest.raises(CwfaHipError):
        ops.chain_inv_var(None, dev, 1.0, shape=shape, std_scale=-1.0)
    gin = [ops.stage(torch.randn(shape).cuda(), None, gin=True)]
    with pytest.raises(CwfaHipError):
        ops.chain_inv_var(None, gin, 1.0, shape=shape)
    with pytest.raises(ValueError):
        ops.chain_inv_var(None, [ops.stage(None, None)] * 9, 1.0, shape=shape)
    with pytest.raises(ValueError):
        ops.chain_inv_var(None, dev, 1.0)                     # neither var_low nor a shape


# ------------------------------------------------------------------------------------------------ the reference fixture
def _fixture_step():
    from cwfa_amd import networks as N
    from test_host_logic import build_step
    fx = load_golden("g24_posterior")
    keep = N.networks_n_chans
    try:
        _, g = build_step("CAT", int(fx["ix"]), D=int(fx["D"]), H=int(fx["H"]), W=int(fx["W"]), n_ch=int(fx["n_ch"]), cond_ch=int(fx["cond_ch"]))
    finally:
        N.networks_n_chans = keep
    g.load_state_dict(sd_of(fx))
    for i, m in enumerate(g.module_list):
        if f"meta/axis_{i}" in fx:
            assert int(m.axis) == int(fx[f"meta/axis_{i}"])
    return fx, g.eval().cuda()


def test_reference_fixture():
    """The package's step with the fixture's weights and conditions: stages from the plan's inverse_stages, the closed-form variance
    against the reference's var_factor = (step([1, low]) - step([0, low]))^2, the mean against its x0."""
    from cwfa_amd import ops
    from cwfa_amd.FrEIA.framework import _CatStepPlan
    fx, g = _fixture_step()
    assert type(g._plan) is _CatStepPlan
    c = [torch.from_numpy(fx["c0"]).cuda(), torch.from_numpy(fx["c1"]).cuda()]
    low = torch.from_numpy(fx["low"]).cuda()
    with torch.no_grad():
        stages, tabs = g._plan.inverse_stages(c)
        var = ops.chain_inv_var(None, stages, 1.0, shape=tuple(low.shape), tables=tabs)
        x0 = ops.chain_inv(None, low, stages, tables=tabs)
        again, _ = g([None, low], c=c, rev=True, jac=False)
    _close("fixture var_factor", var, fx["var_factor"], FIX_BOUND)
    assert _pairs_equal(var)
    assert_close(x0, fx["x0"], TOL, "fixture x0")
    assert torch.equal(x0, again)                            # the plan's own run makes the same launch


def test_samples_agree_with_closed_form():
    """One step at (1, 3, 24, 64), T = 1, S = 256 draws of sample_z_truncated through the existing ops.chain_inv.  r = mean over the
    N = 2*3*24*64 voxels of (sample variance / closed-form variance).  Every voxel is a scaled truncated normal with kurtosis
    below 3 (1.94 at T = 1), so sd(r_voxel) <= sqrt(2 / (S - 1)); only the two voxels of a pair are dependent, so
    sd(r) <= sqrt(4 / ((S - 1) N)) = 1.3e-3.  Required: |r - 1| <= 6 sd(r) = 7.8e-3; each of the formula mistakes named in the
    module docstring moves r by a factor of two or more."""
    from cwfa_amd import CWFA, ops
    shape = (1, 3, 24, 64)
    S = 256
    ref, dev, _ = make_chain(shape, [None, 3, 1, 2, 3, 1], 85)
    low = torch.randn(shape, generator=torch.Generator().manual_seed(86)).cuda()
    torch.manual_seed(87)
    xs = torch.stack([ops.chain_inv(CWFA.sample_z_truncated(low, device="cuda", temperature=1), low, dev) for _ in range(S)]).double()
    closed = ops.chain_inv_var(None, dev, CWFA.truncated_normal_variance(1), shape=shape).double()
    mean0 = ops.chain_inv(None, low, dev).double()
    sample_var = xs.var(dim=0, unbiased=True)
    N = closed.numel()
    r = float((sample_var / closed).mean())
    sd = math.sqrt(4.0 / ((S - 1) * N))
    print(f"[posterior] samples vs closed form: r = {r:.6f}, |r - 1| = {abs(r - 1):.3e}, 6 sd = {6 * sd:.3e}")
    assert abs(r - 1.0) <= 6.0 * sd
    # and the sample mean around the closed-form mean: each voxel's mean has variance closed / S
    zscore = (xs.mean(0) - mean0) / (closed / S).sqrt()
    assert float(zscore.abs().max()) < 6.0


# ------------------------------------------------------------------------------------------------ the pyramid
def _pyramid(block_type="CAT"):
    from cwfa_amd import CWFA
    torch.manual_seed(0)
    np.random.seed(0)
    D, side, S = 16, 64, 3
    conv_inn, cond_nets = CWFA.build_networks(D, side, S, block_type=block_type, internal_chans=8, cond_chans=4, with_lrnn=False)
    g = torch.Generator().manual_seed(1)
    cond_input = torch.randn(1, 29, side, side, generator=g).cuda()
    mean_cache = [(0.1 * torch.randn(1, D // 2 ** (n + 1), side, side, generator=g)).cuda() for n in range(S - 1)]
    low = torch.randn(1, D // 2 ** (S - 1), side, side, generator=g).cuda()
    return conv_inn, cond_nets, cond_input, mean_cache, low


def _by_hand(conv_inn, cond_nets, cond_input, mean_cache, low, latents):
    """The reconstruction loop with given latents per step (execution order; None = zeros), through the graphs themselves."""
    up = low
    with torch.no_grad():
        for i, n in enumerate(range(len(conv_inn) - 1, -1, -1)):
            c = [cond_nets[n](cond_input)[-1], mean_cache[n]]
            up, _ = conv_inn[n]([latents[i], up], c=c, rev=True, jac=False)
    return up


def test_pyramid_moments():
    from cwfa_amd import CWFA
    conv_inn, cond_nets, cond_input, mean_cache, low = _pyramid()
    with torch.no_grad():
        want_mean = CWFA.inverse_pass(conv_inn, cond_nets, cond_input, mean_cache, low=low, temperature=0, keep_all=True)
    T = 0.8
    mean, std = CWFA.posterior_moments(conv_inn, cond_nets, cond_input, mean_cache, low=low, temperature=T)
    assert torch.equal(mean, want_mean[-1])
    # by hand: per level one pass with that level's z = 1 and every other z = 0
    x0 = _by_hand(conv_inn, cond_nets, cond_input, mean_cache, low, [None, None]).double()
    assert torch.equal(x0.float(), mean)
    total = torch.zeros_like(x0)
    shapes = [(1,) + tuple(conv_inn[n].global_out_shapes[0]) for n in range(len(conv_inn) - 1, -1, -1)]
    for i in range(len(conv_inn)):
        lat = [torch.zeros(s, device="cuda") for s in shapes]
        lat[i] = torch.ones(shapes[i], device="cuda")
        total += (_by_hand(conv_inn, cond_nets, cond_input, mean_cache, low, lat).double() - x0) ** 2
    want_std = (CWFA.truncated_normal_variance(T) * total).sqrt()
    # the by-hand differences cancel in fp32: each (x_n - x_0) carries 2^-24 |x| / |x_n - x_0| of relative error on top of the kernel's
    _close("pyramid std", std, want_std, FIX_BOUND)
    # std_scale and keep_all
    means, stds = CWFA.posterior_moments(conv_inn, cond_nets, cond_input, mean_cache, low=low, temperature=T, std_scale=2.5, keep_all=True)
    assert len(means) == len(stds) == len(conv_inn) + 1
    for a, b in zip(means, want_mean):
        assert torch.equal(a, b)
    assert not stds[0].any() and stds[0].shape == low.shape
    _close("std_scale in the last launch", stds[-1], 2.5 * std.double(), 4 * 2.0 ** -24)
    assert all(s.shape == m.shape for s, m in zip(stds, means))
    # the intermediate level is unscaled: the coarser step alone
    m1, s1 = CWFA.posterior_moments(conv_inn[1:], cond_nets[1:], cond_input, mean_cache[1:], low=low, temperature=T)
    assert torch.equal(m1, means[1]) and torch.equal(s1, stds[1])
    # temperature 0: no spread at all
    _, s0 = CWFA.posterior_moments(conv_inn, cond_nets, cond_input, mean_cache, low=low, temperature=0)
    assert not s0.any()


def _count_calls(conv_inn, cond_nets, counts, undo):
    """Count every evaluation of a condition net (forward hook) and of a flow sub-network: the fused plans call a sub-network's
    ``affine_parts`` where it has one (no module ``__call__``, so no forward hook fires), its ``forward`` otherwise."""
    for n, net in enumerate(cond_nets):
        h = net.register_forward_hook(lambda m, i, o, key=f"omega{n}": counts.__setitem__(key, counts.get(key, 0) + 1))
        undo.append(h.remove)
    for n, g in enumerate(conv_inn):
        for i, m in enumerate(g.module_list):
            sub = getattr(m, "subnet", None)
            if sub is None:
                continue
            key = f"step{n}/module{i}"
            counts[key] = 0
            if hasattr(sub, "affine_parts"):
                orig = sub.affine_parts

                def counted(*a, _orig=orig, _key=key, **k):
                    counts[_key] += 1
                    return _orig(*a, **k)
                sub.affine_parts = counted
                undo.append(lambda s=sub: s.__dict__.pop("affine_parts", None))
            h = sub.register_forward_hook(lambda mod, i_, o, _key=key: counts.__setitem__(_key, counts[_key] + 1))
            undo.append(h.remove)


@pytest.mark.parametrize("n_samples", [1, 3])
def test_pyramid_samples(n_samples):
    from cwfa_amd import CWFA
    conv_inn, cond_nets, cond_input, mean_cache, low = _pyramid()
    counts, undo = {}, []
    _count_calls(conv_inn, cond_nets, counts, undo)
    try:
        torch.manual_seed(5)
        xs, zs = CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, n_samples, low=low, temperature=0.7, return_z=True)
    finally:
        for u in undo:
            u()
    # every network ONCE, whatever n_samples is: 2 condition nets, 5 sub-networks per step
    assert len(counts) == 2 + 2 * 5 and all(v == 1 for v in counts.values()), counts
    assert xs.shape == (n_samples, 1, 16, 64, 64) and len(zs) == 2 and all(z.shape[0] == n_samples for z in zs)
    assert all(float(z.abs().max()) <= 0.7 for z in zs)
    for i in range(n_samples):
        assert torch.equal(xs[i], _by_hand(conv_inn, cond_nets, cond_input, mean_cache, low, [z[i] for z in zs]))
    if n_samples > 1:
        assert not torch.equal(xs[0], xs[1])
    # temperature 0: copies of the mean
    with torch.no_grad():
        mean = CWFA.inverse_pass(conv_inn, cond_nets, cond_input, mean_cache, low=low, temperature=0)
    x0, z0 = CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, n_samples, low=low, temperature=0, return_z=True)
    assert all(torch.equal(x0[i], mean) for i in range(n_samples)) and all(z is None for z in z0)


def test_other_block_types_raise():
    from cwfa_amd import CWFA
    conv_inn, cond_nets, cond_input, mean_cache, low = _pyramid("GLOW")
    with pytest.raises(NotImplementedError, match="affine"):
        CWFA.posterior_moments(conv_inn, cond_nets, cond_input, mean_cache, low=low)
    with pytest.raises(NotImplementedError, match="affine"):
        CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, 2, low=low)
    with pytest.raises(NotImplementedError):
        conv_inn[0]._plan.inverse_stages([cond_nets[0](cond_input)[-1], mean_cache[0]])
