"""GPU (MI355X): the likelihood maps of a CAT pyramid -- cwfa_chain_nll_map_f32 in both of its forms and
cwfa_nll_compose_f32 against the float64 restatement (tests/nllmap_ref.py) on the same fp32 inputs, the positions through the
sampler, the reference fixture g24_posterior, and CWFA.nll_maps / zscore_coverage on a pyramid.

z.  Measure and scale are those of tests/test_gpu_chain_dispatch.py: e = max_p |z - z_ref|[p] / M[p], M = chain_ref.chain_magnitude on
chain_ref.inverse_stages(stages), read where each position's latent starts (= (|d| + M_o) exp(a): the cancellation in d - o is
relative to it).  With U = 2^-24 the kernel's z = fl(fl(fl(fl(e - o') c) - o) expf(a)) adds, relative to M,
    per stage with s    c_k + (S log2(e) [16-byte form] + 4) U     that file's stage budget for o <- fl(fl(o - T) E), E = exp(-s (1 + ..)):
                        c_k = clamp * a_kind is the absolute error of s (a_ATAN = 0.636 * 1.9e-7, a_TANH = 2.5e-7, a_NONE = 2 A U,
                        a_SIGMOID = (7 + A / 2) U);  A = max |raw * pre| and S = max |s| are taken from the case's own data (the
                        coefficients of test_gpu_posterior.make_chain are not clipped)
                        + c_k       the same error of s once more, in a (an absolute error of a is a relative error of exp(a))
                        + j S U     the rounding of the running sum at the j-th stage that has an s, |a| <= j S (none at the first:
                                    0 + s is exact)
    per stage without s 2 U with a shift, nothing without
    once                2 U + 2.4e-8 for the Haar pair (two roundings and fl(1 / sqrt 2), which is off by 2.4e-8 relative), U for d - o,
                        2 U for expf (one ulp) and U for the product
The errors of earlier stages travel by the same factors as M, so the budgets add.  Seven ATAN stages in the 16-byte form with S = 2:
9.9e-6; every case is below 1e-5 at S = 2, A = 4 pre (asserted at import) and again on its own data when it runs.  A wrong sign of
s, a dropped gather or a wrong t convention sit at 0.1 and above.

nll is checked on the kernel's OWN z:  |nll - (z_got^2 / 2 - a_ref)| <= (n_s + 3) U (z^2 / 2 + sum |s|) + sum c_k  per element: the
square (2 U of z^2 / 2), the difference (U of z^2 / 2 + |a|), n_s - 1 roundings of the running sum (each U sum |s| at most) and the
absolute errors of the s values.  nll_sum: the float64 sum of the kernel's own map to 1e-12 of sum |nll|, accumulated onto a
non-zero start.  low: bit-equal to ops.chain_fwd's.

The reference fixture and the pyramid add the sub-networks' arithmetic: FIX_* are 4 x the figures measured once on an MI355X (the
project's margin for another compiler release), the pyramid's sums have the bound derived at test_pyramid.

Largest figures measured on an MI355X (every test prints its own next to its bound, pytest -s):
  z, 16-byte form    6.9e-7 (six stages, two column gathers; bound 7.6e-6), 7.8e-7 (seven stages; 9.1e-6), 3.9e-7 (all clamp kinds; 8.0e-6)
  z, general form    4.2e-7 / 5.1e-7 (the two small shapes; 6.7e-6), 6.0e-7 on the shifted view, 3.6e-7 (all clamp kinds); general against
                     16-byte form 3.7e-7
  nll                at most 2.0e-7 of z^2 / 2 + sum |s|, 0.22 of its bound; nll_sum exact to the last bit printed
  positions          max |z - drawn| 4.9e-5, 0.024 of the round-trip budget; coverage 0.68213 / 0.95413 / 0.99734, the restatement's own
  fixture            z 4.62e-6, nll on the kernel's z 2.78e-5, max |z - z*| 3.2e-6 (g spans 0.0445 .. 30.2)
  pyramid            z 3.2e-7 per step; sums against 0.5 sumsq - logdet 5.9e-4 and 7.9e-4 of 2.7e4 and 2.9e4 (bound 0.38 / 0.41: the
                     worst case over 32 768 / 16 384 elements); volume map total against the sums 7.5e-6"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import chain_ref as CR
import nllmap_ref as R
import posterior_ref as PR
from conftest import load_golden                                                        # noqa: F401  (used through _fixture_step)
from test_gpu_chain_dispatch import ATAN_ERR, LOG2E, TANH_ERR, U, low_fp32
from test_gpu_conv_dispatch import nan_around, untouched_outside
from test_gpu_posterior import _fixture_step, _pyramid, make_chain
from test_gpu_sampler import value_bound as sampler_bound

pytestmark = pytest.mark.gpu

C_ERR = abs(float(np.float32(1.0 / math.sqrt(2.0))) * math.sqrt(2.0) - 1.0)              # fl(1 / sqrt 2) against 1 / sqrt 2: 2.4e-8
ONCE = 6 * U + C_ERR
AXES6 = [3, 1, None, 2, 3, 1]
AXES_COL2 = [None, 3, 1, 2, 3, 1]
AXES7 = [3, 1, None, 2, 3, 1, 2]
KINDS = dict(no_s=(4,), no_t=(1,), kinds=["NONE", "ATAN", "TANH", "SIGMOID", "ATAN", "TANH"], pres=[1.0, 1.0, 0.1, 1.0, 1.0, 1.0],
             clamps=[0.5, 2.0, 2.0, 1.5, 2.0, 1.0])

FIX_Z_MEASURED = 4.63e-6      # the reference fixture, measured once on an MI355X: z on M = (|d| + |o|) / g
FIX_NLL_MEASURED = 2.78e-5    # and nll on the kernel's own z, relative to z^2 / 2 + |log g| (where both are small, a's absolute error shows)


# ------------------------------------------------------------------------------------------------ the bound
def clamp_err(kind, clamp, A):
    """absolute error of the clamped s for raw coefficients with |raw * pre| <= A (tests/test_gpu_chain_dispatch.py)"""
    return clamp * {"ATAN": 0.636 * ATAN_ERR, "TANH": TANH_ERR, "SIGMOID": (7 + A / 2) * U, "NONE": 2 * A * U}[kind]


def z_bound(params, fast, S, clamp_terms=True):
    """params: per stage (kind, clamp, A, has_s, has_t) in execution order -- module docstring"""
    tot, j = ONCE, 0
    for kind, clamp, A, has_s, has_t in params:
        if not has_s:
            tot += 2 * U if has_t else 0.0
            continue
        j += 1
        tot += (S * LOG2E * bool(fast) + 4) * U + (j * S * U if j > 1 else 0.0)
        if clamp_terms:
            tot += 2 * clamp_err(kind, clamp, A)
    return tot


def fwd_bound_no_clamp(params, S):
    """the forward chain's budget of tests/test_gpu_chain_dispatch.py (16-byte form) without the error of s itself"""
    return sum((S * LOG2E + 4) * U if p[3] else (2 * U if p[4] else 0.0) for p in params) + 2 * U


def static_params(n, kinds=None, pres=None, clamps=None, no_s=(), no_t=()):
    return [((kinds or ["ATAN"] * n)[k], (clamps or [2.0] * n)[k], 4.0 * (pres or [1.0] * n)[k], k not in no_s, k not in no_t) for k in range(n)]


for _p in (static_params(6), static_params(5), static_params(7), static_params(6, **KINDS)):
    assert ONCE < z_bound(_p, True, 2.0) < 1e-5, z_bound(_p, True, 2.0)
assert z_bound([], True, 2.0) == ONCE


def data_params(ref):
    """(params, S, sum of c_k, number of stages with s) of a case's reference stages, A and S from the data"""
    params, S, csum, ns = [], 0.0, 0.0, 0
    for st in ref:
        has_s = st.get("s_raw") is not None
        A = float((st["s_raw"] * torch.tensor(st["pre"], dtype=torch.float32)).abs().max()) if has_s else 0.0
        params.append((st["kind"], st["clamp"], A, has_s, st.get("t") is not None))
        if has_s:
            S = max(S, float(PR.stage_s(st).abs().max()))
            csum += clamp_err(st["kind"], st["clamp"], A)
            ns += 1
    return params, S, csum, ns


# ------------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


def volume(shape, seed):
    B, Cc, H, W = shape
    return torch.randn((B, 2 * Cc, H, W), generator=torch.Generator().manual_seed(seed))


def reference(x, ref):
    """nllmap_ref.chain_nll_map with M taken from the existing restatement: chain_ref's forward magnitude walk on the inverse of the stages, read where
    each position's latent starts (the same numbers, asserted)"""
    m = R.chain_nll_map(x, ref)
    M = R.at_positions(CR.chain_magnitude(CR.inverse_stages(ref), x=x), ref)
    assert float(((M - m["M"]).abs() / M.clamp_min(1e-300)).max()) < 1e-10
    m["M"] = M
    return m


def check_z(what, z, m, bound):
    e = float(((z.double().cpu() - m["z"]).abs() / m["M"].clamp_min(1e-300)).max())
    print(f"[nllmap] {what}: z  e = {e:.3e} (bound {bound:.3e})")
    assert bool(torch.isfinite(z).all()) and bound < 1e-5
    assert e <= bound, f"{what}: max |z - z_ref| / M = {e:.3e} > {bound:.3e}"
    return e


def check_nll(what, nll, z, m, ns, csum):
    zg = z.double().cpu()
    err = (nll.double().cpu() - (0.5 * zg * zg - m["a"])).abs()
    scale = 0.5 * zg * zg + m["sabs"]
    lim = (ns + 3) * U * scale + csum
    worst = float((err / lim.clamp_min(1e-300)).max())
    rel = float((err / scale.clamp_min(1e-300)).max())
    print(f"[nllmap] {what}: nll error {float(err.max()):.3e} absolute, {rel:.3e} of z^2/2 + sum|s|, {worst:.3f} of its bound "
          f"({(ns + 3) * U:.3e} relative + {csum:.3e})")
    assert bool((err <= lim).all()), f"{what}: nll off by {worst:.3f} of its bound"


def check_sum(what, acc, start, nll):
    want = nll.double().flatten(1).sum(1)
    tot = nll.double().abs().flatten(1).sum(1)
    err = (acc - start - want).abs()
    print(f"[nllmap] {what}: nll_sum error {float((err / tot).max()):.3e} of sum |nll| (bound 1e-12)")
    assert bool((err <= 1e-12 * (tot + start.abs())).all()), (what, err.tolist())


def run_case(what, shape, axes, seed, fast, tables=False, x_dev=None, **kw):
    """all outputs of one launch against the float64 reference; returns (nll, low, z, reference dict, bound)"""
    from cwfa_amd import ops
    ref, dev, perms = make_chain(shape, axes, seed, **kw)
    x = volume(shape, seed + 1000)
    xd = x.cuda() if x_dev is None else x_dev(x)
    m = reference(x, ref)
    params, S, csum, ns = data_params(ref)
    bound = z_bound(params, fast, S)
    start = torch.arange(1, shape[0] + 1, dtype=torch.float64, device="cuda") * 3.5
    acc = start.clone()
    tabs = ops.chain_tables(perms, None, *shape[1:], "cuda") if tables else None
    nll, low, z = ops.chain_nll_map(xd, dev, tables=tabs, want_z=True, nll_sum=acc)
    check_z(what, z, m, bound)
    check_nll(what, nll, z, m, ns, csum)
    check_sum(what, acc, start, nll)
    assert torch.equal(low, ops.chain_fwd(x.cuda(), [])[1]) and torch.equal(low.cpu(), low_fp32(x))
    return nll, low, z, m, bound, (ref, dev, perms, x)


# ------------------------------------------------------------------------------------------------ the kernel's two forms
@pytest.mark.parametrize("shape,axes", [((2, 3, 5, 7), AXES6), ((1, 6, 9, 12), [None, 1, 2, 3, 1])])
def test_general_form(shape, axes):
    """Odd sizes and W < 64: the pull kernel (648 positions: a partial last block)."""
    run_case(f"general {shape}", shape, axes, sum(shape), False)


def test_rows4_form_with_and_without_tables():
    """(2, 3, 24, 64): 16 rows per block, so the second block is half dead (its sums must not count); six stages with TWO column
    gathers (both exchange buffers), a channel gather and a row gather; composed tables or the dependent walk: bitwise the same."""
    shape = (2, 3, 24, 64)
    a = run_case(f"rows4 {shape}", shape, AXES_COL2, 177, True)
    b = run_case(f"rows4 {shape} tables", shape, AXES_COL2, 177, True, tables=True)
    assert all(torch.equal(u, v) for u, v in zip(a[:3], b[:3]))


def test_more_than_six_stages():
    from cwfa_amd import ops
    shape = (1, 3, 16, 64)
    nll, low, z, _, _, (ref, dev, perms, x) = run_case("seven stages", shape, AXES7, 178, True)
    again = ops.chain_nll_map(x.cuda(), dev, tables=ops.chain_tables(perms, None, *shape[1:], "cuda"), want_z=True)
    assert torch.equal(again[0], nll) and torch.equal(again[1], low) and torch.equal(again[2], z)


def test_general_against_rows4_form():
    """The same chain on an x view shifted by one float (not 16-byte aligned) falls to the general form.  The two forms differ in
    the exponential of o's stages alone (expf / the fast one); every other operation is the same fp32 expression on the same
    operands, so their difference stays inside the 16-byte form's budget."""
    shape = (1, 3, 16, 64)

    def shifted(x):
        buf = torch.empty(x.numel() + 4, device="cuda")
        v = buf[1:x.numel() + 1].view(x.shape)
        v.copy_(x)
        assert v.data_ptr() % 16 == 4
        return v
    a = run_case("aligned run", shape, AXES_COL2, 179, True)
    g = run_case("shifted run (general form)", shape, AXES_COL2, 179, False, x_dev=shifted)
    e = float(((a[2].double().cpu() - g[2].double().cpu()).abs() / a[3]["M"]).max())
    print(f"[nllmap] general vs 16-byte form: e = {e:.3e} (bound {a[4]:.3e})")
    assert e <= a[4] and e > 0.0            # (bit-equal would mean the shifted run took the 16-byte form after all)
    assert torch.equal(a[1], g[1])


@pytest.mark.parametrize("shape,fast", [((2, 3, 5, 7), False), ((1, 3, 16, 64), True)])
def test_stage_kinds(shape, fast):
    """All four clamp kinds, pre_scale = 0.1, an s-less and a t-less stage, in both forms."""
    run_case(f"stage kinds {shape}", shape, [3, 1, 2, None, 3, 1], 180, fast, **KINDS)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 24, 64)])
def test_exact_cases(shape):
    from cwfa_amd import ops
    x = volume(shape, 181)
    c32 = torch.tensor(0.70710678118654752440, dtype=torch.float32)
    d = (x[:, 0::2] - x[:, 1::2]) * c32
    # the empty chain and a chain of gathers only: a = o = 0, so z is the detail itself and nll = z^2 / 2, bit for bit
    gathers = [ops.stage(None, None, perm=torch.randperm(shape[3], generator=torch.Generator().manual_seed(5)).cuda(), axis=3),
               ops.stage(None, None), ops.stage(None, None, perm=torch.randperm(shape[1], generator=torch.Generator().manual_seed(6)).cuda(), axis=1)]
    for stages in ([], gathers):
        acc = torch.zeros(shape[0], dtype=torch.float64, device="cuda")
        nll, low, z = ops.chain_nll_map(x.cuda(), stages, want_z=True, nll_sum=acc)
        assert torch.equal(z.cpu(), d) and torch.equal(nll.cpu(), 0.5 * d * d) and torch.equal(low.cpu(), low_fp32(x))
        assert float((acc.cpu() - (0.5 * d * d).double().flatten(1).sum(1)).abs().max()) <= 1e-12 * float((0.5 * d * d).double().sum())
    # every combination of the nullable outputs: what is requested is bit-equal to the full launch
    _, dev, _ = make_chain(shape, AXES6, 182)
    full = ops.chain_nll_map(x.cuda(), dev, want_low=True, want_z=True, want_nll=True)
    for want in itertools.product([False, True], repeat=3):
        if not any(want):
            continue
        acc = torch.zeros(shape[0], dtype=torch.float64, device="cuda")
        got = ops.chain_nll_map(x.cuda(), dev, want_nll=want[0], want_low=want[1], want_z=want[2], nll_sum=acc if want[2] else None)
        for on, g_, f_ in zip(want, got, full):
            assert (g_ is None and not on) or (on and torch.equal(g_, f_)), want
    acc = torch.full((shape[0],), 2.0, dtype=torch.float64, device="cuda")           # the sum alone
    assert ops.chain_nll_map(x.cuda(), dev, want_low=False, want_z=False, want_nll=False, nll_sum=acc) == (None, None, None)
    check_sum(f"sum alone {shape}", acc, torch.full_like(acc, 2.0), full[0])


@pytest.mark.parametrize("off", [0, 1], ids=["rows4", "general"])
def test_channel_slices_of_nan_tensors(off):
    """x read and low / z / nll written as channel slices of NaN-filled tensors, through the library entry point itself (off = 1:
    x one float past the 16-byte grid -- the general form): nothing outside the slices changes, no NaN appears inside."""
    from cwfa_amd import _lib, ops
    shape = (2, 3, 24, 64)
    B, Cc, H, W = shape
    _, dev, _ = make_chain(shape, AXES_COL2, 183)
    x = volume(shape, 184)
    xv, xflat = nan_around((B, 2 * Cc, H, W), 1, 2, off)
    xv.copy_(x)
    outs = [nan_around(shape, b, a) for b, a in ((2, 1), (1, 1), (0, 3))]
    ch, keep = ops._chain(dev)
    acc = torch.zeros(B, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().cwfa_chain_nll_map_f32(C.c_void_p(xv.data_ptr()), *(C.c_void_p(v.data_ptr()) for v, _ in outs), C.byref(ch), B, Cc,
                                                 H, W, xv.stride(0), *(v.stride(0) for v, _ in outs), C.c_void_p(acc.data_ptr()),
                                                 ops._stream()), "chain_nll_map")
    torch.cuda.synchronize()
    nll, low, z = ops.chain_nll_map(x.cuda(), dev, want_z=True)
    for (v, flat), want in zip(outs, (low, z, nll)):
        assert untouched_outside(v, flat) and not v.isnan().any()
        if off == 0:
            assert torch.equal(v, want)
    assert untouched_outside(xv, xflat) and torch.equal(xv, x.cuda())
    assert torch.equal(outs[0][0], low)


def test_errors():
    from cwfa_amd import ops
    from cwfa_amd._lib import CwfaHipError
    shape = (1, 2, 4, 8)
    _, dev, _ = make_chain(shape, [3, 1], 185)
    x = volume(shape, 186).cuda()
    with pytest.raises(CwfaHipError, match="GIN"):
        ops.chain_nll_map(x, [ops.stage(torch.randn(shape).cuda(), None, gin=True)])
    with pytest.raises(CwfaHipError, match="no output"):
        ops.chain_nll_map(x, dev, want_low=False, want_z=False, want_nll=False)
    with pytest.raises(ValueError):
        ops.chain_nll_map(x, [ops.stage(None, None)] * 9)
    with pytest.raises(ValueError):
        ops.chain_nll_map(x[:, :3], dev)
    with pytest.raises(ValueError):
        ops.chain_nll_map(x, dev, nll_sum=torch.zeros(2, dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        ops.chain_nll_map(x, dev, nll_sum=torch.zeros(1, device="cuda"))


# ------------------------------------------------------------------------------------------------ compose
@pytest.mark.parametrize("shape,L", [((2, 16, 3, 5), 3), ((1, 16, 24, 64), 2), ((2, 8, 16, 64), 3), ((1, 256, 1, 4), 8)])
def test_compose(shape, L):
    """odd pixels (element by element) and 16-byte rows, L = 1 .. 8: bit-equal to the same fp32 expression on the CPU; level views
    with a batch stride of their own."""
    from cwfa_amd import ops
    B, D, H, W = shape
    g = torch.Generator().manual_seed(187)
    levels = [torch.randn(B, D >> (n + 1), H, W, generator=g) for n in range(L)]
    want = R.compose(levels, torch.float32)
    got = ops.nll_compose([lv.cuda() for lv in levels])
    assert got.shape == shape and torch.equal(got.cpu(), want)
    wide = torch.randn(B, D, H, W, generator=g).cuda()                   # the finest level as a channel slice of a larger tensor
    wide[:, 1:1 + D // 2] = levels[0].cuda()
    assert torch.equal(ops.nll_compose([wide[:, 1:1 + D // 2]] + [lv.cuda() for lv in levels[1:]]), got)
    tot = sum(lv.double().sum() for lv in levels)
    assert abs(float(got.double().sum()) - float(tot)) <= (L - 1) * U * float(sum(lv.double().abs().sum() for lv in levels)) + 1e-9
    with pytest.raises(ValueError):
        ops.nll_compose([levels[0].cuda(), levels[0].cuda()])          # the second level has the first one's channels


# ------------------------------------------------------------------------------------------------ positions, through the sampler
POS_SHAPE, POS_SEED = R.POS_SHAPE, R.POS_SEED


def test_positions_through_the_sampler():
    """x = one draw of ops.chain_inv_samples at T = 1: the generator indexes its latents by the position they ARRIVE at, so the z-map
    of x is ops.rand_trunc_normal itself.  Budget (the round trip of tests/test_gpu_chain_dispatch.py): the sampler's own bound on x
    relative to M_x (tests/test_gpu_sampler.py) moves d by sqrt 2 * that and z by exp(a) times it; the map adds its z bound on M."""
    from cwfa_amd import ops
    shape = POS_SHAPE
    ref, dev, _ = make_chain(shape, AXES_COL2, 188)
    low = torch.randn(shape, generator=torch.Generator().manual_seed(189))
    xs, zs = ops.chain_inv_samples(low.cuda(), dev, 1, 1.0, POS_SEED, return_z=True)
    drawn = ops.rand_trunc_normal((1,) + shape, 1.0, POS_SEED)[0]
    _, _, z = ops.chain_nll_map(xs[0], dev, want_low=False, want_z=True, want_nll=False)
    params, S, _, _ = data_params(ref)
    m = reference(xs[0].cpu(), ref)
    Mx = CR.chain_magnitude(ref, z=zs[0].cpu(), low=low, inverse=True)[:, 0::2]
    lim = z_bound(params, True, S) * m["M"] + math.sqrt(2.0) * sampler_bound(AXES_COL2) * Mx * torch.exp(m["a"])
    err = (z.double().cpu() - drawn.double().cpu()).abs()
    print(f"[nllmap] positions: max |z - drawn| = {float(err.max()):.3e}, {float((err / lim).max()):.3f} of the round-trip budget")
    assert bool((err <= lim).all())
    assert torch.equal(R.at_positions(zs[0].cpu(), ref), drawn.cpu())        # the sampler's own statement of where its latents start


def test_zscore_coverage_of_posterior_samples():
    """8 draws at T = inf, 36 864 z-scores: the fraction inside +-k is erf(k / sqrt 2) to 6 sqrt(p (1 - p) / N) (the numpy restatement
    of the generator is inside that band for this seed: tests/test_nllmap_cpu.py)."""
    from cwfa_amd import CWFA, ops
    shape = POS_SHAPE
    _, dev, _ = make_chain(shape, AXES_COL2, 188)
    low = torch.randn(shape, generator=torch.Generator().manual_seed(189)).cuda()
    xs = ops.chain_inv_samples(low, dev, 8, math.inf, POS_SEED)
    z = torch.stack([ops.chain_nll_map(xs[i], dev, want_low=False, want_z=True, want_nll=False)[2] for i in range(8)])
    obs, exp = CWFA.zscore_coverage([z])
    N = z.numel()
    assert N == 36864 and obs.shape == (1, 3) and obs.is_cuda
    for k, o, p in zip((1, 2, 3), obs[0].tolist(), exp.tolist()):
        band = 6.0 * math.sqrt(p * (1.0 - p) / N)
        print(f"[nllmap] coverage |z| <= {k}: {o:.5f} (normal {p:.5f}, band {band:.5f})")
        assert abs(o - p) <= band


# ------------------------------------------------------------------------------------------------ the reference fixture
FIX_Z_BOUND, FIX_NLL_BOUND = 4 * FIX_Z_MEASURED, 4 * FIX_NLL_MEASURED
assert FIX_Z_BOUND < 1e-3 and FIX_NLL_BOUND < 1e-3


def test_reference_fixture():
    """The package's step with the fixture's weights and conditions.  From the REFERENCE's own numbers: g = sqrt(2 var_factor[2c]) (the
    response of a pair to its latent) and o = the detail of its z = 0 reconstruction x0.  A volume with known z-scores z* (uniform in
    [-3, 3]) is d = g z* + o on the fixture's low; rounded to fp32 its detail has z_ref = (d(x32) - o) / g and nll_ref = z_ref^2 / 2 +
    log g.  Measure as above with M = (|d| + |o|) / g; nll on the kernel's own z, relative to z^2 / 2 + |log g|."""
    from cwfa_amd import ops
    fx, g_ = _fixture_step()
    c = [torch.from_numpy(fx["c0"]).cuda(), torch.from_numpy(fx["c1"]).cuda()]
    low = torch.from_numpy(fx["low"]).double()
    g = (2.0 * torch.from_numpy(fx["var_factor"]).double()[:, 0::2]).sqrt()
    x0 = torch.from_numpy(fx["x0"]).double()
    o = (x0[:, 0::2] - x0[:, 1::2]) / math.sqrt(2.0)
    print(f"[nllmap] fixture: g spans {float(g.min()):.3g} .. {float(g.max()):.3g}")
    zstar = torch.rand(g.shape, generator=torch.Generator().manual_seed(190), dtype=torch.float64) * 6.0 - 3.0
    d = g * zstar + o
    x = torch.empty_like(x0)
    x[:, 0::2], x[:, 1::2] = (low + d) / math.sqrt(2.0), (low - d) / math.sqrt(2.0)
    x32 = x.float()
    d32 = (x32[:, 0::2].double() - x32[:, 1::2].double()) / math.sqrt(2.0)
    z_ref = (d32 - o) / g
    with torch.no_grad():
        stages, tabs = g_._plan.inverse_stages(c)
        acc = torch.zeros(x.shape[0], dtype=torch.float64, device="cuda")
        nll, lo, z = ops.chain_nll_map(x32.cuda(), stages, tables=tabs, want_z=True, nll_sum=acc)
    zg = z.double().cpu()
    e = float(((zg - z_ref).abs() / ((d32.abs() + o.abs()) / g)).max())
    en = float(((nll.double().cpu() - (0.5 * zg * zg + g.log())).abs() / (0.5 * zg * zg + g.log().abs())).max())
    print(f"[nllmap] fixture: z  e = {e:.3e} (bound {FIX_Z_BOUND:.3e}), nll on the kernel's z {en:.3e} (bound {FIX_NLL_BOUND:.3e}); "
          f"max |z - z*| = {float((zg - zstar).abs().max()):.3e}")
    assert e <= FIX_Z_BOUND and en <= FIX_NLL_BOUND
    assert torch.equal(lo.cpu(), low_fp32(x32))
    check_sum("fixture", acc, torch.zeros_like(acc), nll)


# ------------------------------------------------------------------------------------------------ the pyramid
def ref_stages(stages):
    """the reference dicts of a plan's device stage list (struct, keep-alive tensors in the order s_raw, t, perm)"""
    from cwfa_amd import _lib
    kinds = {v: k for k, v in _lib.CLAMP.items()}
    out = []
    for st, keep in stages:
        it = iter(keep)
        s_raw = next(it) if st.s_raw else None
        t = next(it) if st.t else None
        perm = next(it) if st.perm else None
        assert (s_raw is None or s_raw.data_ptr() == st.s_raw) and (t is None or t.data_ptr() == st.t)
        assert perm is None or (perm.data_ptr() == st.perm and perm.dtype == torch.int64)
        out.append({"s_raw": None if s_raw is None else s_raw.cpu(), "t": None if t is None else t.cpu(),
                    "perm": None if perm is None else perm.cpu(), "axis": int(st.perm_axis) if perm is not None else None,
                    "kind": kinds[int(st.clamp_kind)], "clamp": float(st.clamp), "pre": float(st.pre_scale), "neg": bool(st.t_neg_div_sqrt2)})
    return out


def test_pyramid():
    """CWFA.nll_maps on a two-step pyramid (side 64: the 16-byte form) against the forward pass it shares its density with.

    sums[b, n] against 0.5 * sumsq - logdet of nll_terms.  Both kernels evaluate the same clamped s bits (the same cwfa_soft_clamp on
    the same coefficients), so the error of s itself cancels; what remains, per element with z*, M, sum |s| from the float64
    restatement on the step's own stage tensors, is
        (zb + fb) M |z*|                   the two z differ from the exact one by zb M (this file's bound without the c_k terms) and fb M
                                           (the forward chain's budget of test_gpu_chain_dispatch.py without them), and z^2 / 2 moves by
                                           |z| times that
        ((n_s + 3) + 8 + 1) U (z*^2 / 2 + sum |s|)     the roundings of nll (module docstring), the forward kernel's fp32 log-det partial
                                           sums (that file's log-det bound) and the plan's fp32 log-det
    summed over the elements, times 1.1 for the second-order terms (the restatement's s differs from the kernels' by c_k <= 3e-7)."""
    from cwfa_amd import CWFA, ops
    from cwfa_amd.networks import omega_first_scope
    conv_inn, cond_nets, cond_input, mean_cache, _ = _pyramid()
    S1 = len(conv_inn)
    vol = torch.randn(1, 16, 64, 64, generator=torch.Generator().manual_seed(191)).cuda()
    full, maps, zmaps, sums, low = CWFA.nll_maps(conv_inn, cond_nets, vol, cond_input, mean_cache, want_z=True)
    assert full.shape == vol.shape and sums.shape == (1, S1) and sums.dtype == torch.float64 and len(maps) == len(zmaps) == S1
    assert [tuple(m.shape) for m in maps] == [(1, 8, 64, 64), (1, 4, 64, 64)] == [tuple(z.shape) for z in zmaps]
    plain = CWFA.nll_maps(conv_inn, cond_nets, vol, cond_input, mean_cache)
    assert plain[2] is None and torch.equal(plain[0], full) and torch.equal(plain[3], sums)
    want, bounds, gt = [], [], vol
    with torch.no_grad(), omega_first_scope(list(cond_nets[:S1]), cond_input):
        for n, g in enumerate(conv_inn):
            c = [cond_nets[n](cond_input)[-1], mean_cache[n]]
            Z, logdet, sumsq = CWFA.nll_terms(g, gt, c)
            want.append(0.5 * float(sumsq[0]) - float(logdet.double().sum()))
            ref = ref_stages(g._plan.inverse_stages(c, tuple(Z[1].shape[1:]), gt.device)[0])
            m = R.chain_nll_map(gt.cpu(), ref)
            params, S, _, ns = data_params(ref)
            zb, fb = z_bound(params, True, S, clamp_terms=False), fwd_bound_no_clamp(params, S)
            scale = 0.5 * m["z"] ** 2 + m["sabs"]
            bounds.append(1.1 * float(((zb + fb) * m["M"] * m["z"].abs() + (ns + 12) * U * scale).sum()))
            # the maps themselves, against the restatement on this step's own coefficients
            check_z(f"pyramid step {n}", zmaps[n], m, z_bound(params, True, S))
            gt = Z[1]
    _, low_fwd = CWFA.forward_nll_pass(conv_inn, cond_nets, vol, cond_input, mean_cache)
    assert torch.equal(low, low_fwd) and torch.equal(low, gt)
    for n in range(S1):
        err = abs(float(sums[0, n]) - want[n])
        print(f"[nllmap] pyramid step {n}: sum {float(sums[0, n]):.6f} vs 0.5 sumsq - logdet {want[n]:.6f}: {err:.3e} (bound {bounds[n]:.3e})")
        assert err <= bounds[n]
        tot = float(maps[n].double().abs().sum())
        assert abs(float(sums[0, n]) - float(maps[n].double().sum())) <= 1e-12 * tot
    # the volume map: the fp32 expression of the compose on the CPU, bit for bit; its total is the pyramid's NLL
    assert torch.equal(full.cpu(), R.compose([m.cpu() for m in maps], torch.float32))
    spread = (S1 - 1) * U * sum(float(m.double().abs().sum()) for m in maps)
    err = abs(float(full.double().sum()) - float(sums.sum()))
    print(f"[nllmap] pyramid: volume map total {float(full.double().sum()):.6f} vs sums {float(sums.sum()):.6f}: {err:.3e} "
          f"(bound {sum(bounds) + spread:.3e})")
    assert err <= sum(bounds) + spread
    assert abs(float(full.double().sum()) - sum(want)) <= sum(bounds) + spread


def test_other_block_types_raise():
    from cwfa_amd import CWFA
    conv_inn, cond_nets, cond_input, mean_cache, _ = _pyramid("GLOW")
    vol = torch.zeros(1, 16, 64, 64, device="cuda")
    with pytest.raises(NotImplementedError, match="affine"):
        CWFA.nll_maps(conv_inn, cond_nets, vol, cond_input, mean_cache)
