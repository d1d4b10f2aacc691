"""GPU (MI355X): the sample-axis posterior sampler -- the device generator (cwfa_rand_uniform_f32,
cwfa_rand_trunc_normal_f32) against the numpy restatement of tests/sampler_ref.py, cwfa_chain_inv_samples_f32 in both of its forms
against the float64 inverse chain of tests/posterior_ref.py on the kernel's own latents, and the seeded paths of CWFA.posterior_samples,
CWFA.posterior_roi_means and CWFA.sample_z_truncated.

Uniforms are bit-equal to the restatement: every step of the map is exact.

Truncated normal: absolute error against the float64 map at the same fp32 argument a = fl(E fl(2u - 1)); what remains is erfinvf, the
product with fl(sqrt 2) and the clamp.  NORMAL_BOUND = 4 x the largest error measured once on an MI355X over T in {0.5, 1, 3, inf}: the
project's margin for another compiler release's erfinvf.  A wrong E, a missing sqrt 2 or a missing clamp are errors of 0.1 and more.

The value bound of the sampler.  Measure and reference are those of tests/test_gpu_chain_dispatch.py: e = max_p |got - ref|[p] / M[p]
with ref = posterior_ref.chain_inv and M = chain_ref.chain_magnitude(inverse=True), both on the kernel's own z_out, U = 2^-24.  The
kernel does not walk the value through the stages: it carries the pair (g, o), g <- fl(g e_k), o <- fl(fl(o - T_k) e_k), and evaluates
fl(fl(g z) + o).  |g| |z| + the magnitude walk of o is M, so the budget is relative to the same M and adds per stage, as derived there,
    clamp * a_kind            the absolute error of s = the relative error of e_k = exp(-s): a_ATAN = 0.636 * 1.9e-7, a_TANH = 2.5e-7
                              (csrc/common.h), a_NONE = 2 A U, a_SIGMOID = (7 + A / 2) U, A = 4 pre (raw coefficients clipped to [-4, 4])
    (S log2(e) + 4) U         S = 2 >= |s|: the fast exponential of the 16-byte form, the exponential itself, the scaling of t and the
                              two roundings of o's stage (the general form calls expf: less)
    1 U                       one more rounding for the running product g e_k
a stage without s is 2 U (o - T and the rounding in T; g * 1 is exact), a stage that only gathers is exact; then 2 U for fl(fl(g z) + o)
and 2 U for the Haar pair.  Seven ATAN stages: 7 * 7.12e-7 + 4 U = 5.2e-6; every case's bound is below 1e-5 (asserted at import).  A
dropped gather, a pair exchanged through the wrong buffer, a wrong t convention or the latent of another position sit at 0.1 to 2.

Largest figures measured on an MI355X (every test prints its own next to the bound, pytest -s):
  truncated normal   1.2e-7 / 2.2e-7 / 6.5e-7 / 8.37e-7 at T = 0.5 / 1 / 3 / inf (bound 3.3e-6)
  values             16-byte form 8.7e-7 (bound 4.5e-6), general form 5.0e-7 (4.5e-6), four waves per row 5.0e-7 (3.8e-6), seven stages
                     6.1e-7 (5.2e-6), all clamp kinds 4.1e-7 (4.7e-6); general against 16-byte form 5.5e-7, latents bit-equal
  statistics         r = 1.000778 and largest z-score 3.597, the restatement's own figures"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import assert_close

import chain_ref as CR
import posterior_ref as R
import sampler_ref as S

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
S_MAX, RAW_MAX = 2.0, 4.0
LOG2E = math.log2(math.e)
ATAN_ERR, TANH_ERR = 1.9e-7, 2.5e-7           # csrc/common.h: cwfa_atan, cwfa_tanh
PRE01 = float(np.float32(0.1))

NORMAL_MEASURED = 8.37e-7     # largest |z - float64 map| over T in {0.5, 1, 3, inf} (at T = inf, |z| up to 4.8; 1.2e-7 / 2.2e-7 / 6.5e-7 at
                              # T = 0.5 / 1 / 3), measured once on an MI355X
NORMAL_BOUND = 4 * NORMAL_MEASURED
assert NORMAL_BOUND < 1e-5
TOL = 1e-4                    # tests/test_gpu_posterior.py: the golden step tests' bound, for the by-hand pyramid
SEED = (0x299f31d0 << 32) | 0xa4093822       # above 2^32: both key words are in use

ATAN6 = [("ATAN", 2.0, 1.0)] * 8
KINDS = [("NONE", 0.5, 1.0), ("ATAN", 2.0, 1.0), ("TANH", 2.0, PRE01), ("SIGMOID", 1.5, 1.0), ("ATAN", 2.0, 1.0), ("TANH", 1.0, 1.0)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ chains and their budget
def stage_budget(kind, clamp, pre, has_s, has_t):
    if not has_s:
        return 2 * U if has_t else 0.0
    A = RAW_MAX * pre
    a = {"ATAN": 0.636 * ATAN_ERR, "TANH": TANH_ERR, "NONE": 2 * A * U, "SIGMOID": (7 + A / 2) * U}[kind]
    return clamp * a + (S_MAX * LOG2E + 4) * U + U


def value_bound(axes, params=ATAN6, no_s=(), no_t=()):
    return sum(stage_budget(*params[k], k not in no_s, k not in no_t) for k in range(len(axes))) + 4 * U


AXES6 = [3, 1, None, 2, 3, 1]
CASES = {                     # name: (shape, axes, params, no_s, no_t)
    "general": ((2, 3, 5, 7), AXES6, ATAN6, (), ()),
    "rows4": ((2, 3, 24, 64), AXES6, ATAN6, (), ()),
    "waves": ((1, 2, 3, 1024), [3, 1, 3, None, 3], ATAN6, (), ()),
    "seven": ((1, 3, 16, 64), [3, 1, None, 2, 3, 1, 2], ATAN6, (), ()),
    "kinds_general": ((2, 3, 5, 7), [3, 1, 2, None, 3, 1], KINDS, (4,), (1,)),
    "kinds_rows4": ((1, 3, 16, 64), [3, 1, 2, None, 3, 1], KINDS, (4,), (1,)),
}
BOUNDS = {name: value_bound(c[1], c[2], c[3], c[4]) for name, c in CASES.items()}
assert all(2 * U < b < 1e-5 for b in BOUNDS.values()), BOUNDS


def make_chain(shape, axes, seed, params=ATAN6, no_s=(), no_t=()):
    """(reference stage dicts on the CPU, ops.stage list on the device, perms per stage for chain_tables) from seeded fp32 draws,
    the raw coefficients clipped to [-RAW_MAX, RAW_MAX]."""
    from cwfa_amd import ops
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(seed)
    ref, dev, perms = [], [], []
    for k, ax in enumerate(axes):
        kind, clamp, pre = params[k]
        s_raw = None if k in no_s else torch.randn(shape, generator=g).clamp_(-RAW_MAX, RAW_MAX)
        t = None if k in no_t else torch.randn(shape, generator=g)
        perm = None if ax is None else torch.randperm([0, Cc, H, W][ax], generator=g)
        neg = k == len(axes) - 1
        st = {"s_raw": s_raw, "t": t, "perm": perm, "axis": ax, "kind": kind, "clamp": clamp, "pre": pre, "neg": neg}
        s = R.stage_s(st)
        assert s is None or float(s.abs().max()) <= S_MAX
        ref.append(st)
        pd = None if perm is None else perm.cuda()
        dev.append(ops.stage(None if s_raw is None else s_raw.cuda(), None if t is None else t.cuda(), kind, clamp, pre_scale=pre,
                             t_neg_div_sqrt2=neg, perm=pd, axis=ax or 1))
        perms.append((pd, ax or 1))
    return ref, dev, perms


def case(name, seed):
    shape, axes, params, no_s, no_t = CASES[name]
    return (shape,) + make_chain(shape, axes, seed, params, no_s, no_t)


def lows(shape, N, seed):
    return torch.randn((N,) + tuple(shape), generator=torch.Generator().manual_seed(seed))


def start_map(ref, shape):
    """idx[p] = linear index (within one sample) of the position where the value arriving at p starts: the gathers walked over an
    index tensor."""
    idx = torch.arange(math.prod(shape)).view(shape)
    for st in ref:
        idx = R._gather(idx, st)
    flat = idx.flatten()
    assert torch.equal(flat.sort().values, torch.arange(flat.numel()))      # a permutation: every start position exactly once
    return flat


def check_z(what, z, ref, shape, T, seed, stream, offset):
    """z_out is bit-equal to the generator's values scattered to the start positions; every element written once."""
    from cwfa_amd import ops
    N = z.shape[0]
    drawn = ops.rand_trunc_normal((N,) + tuple(shape), T, seed, stream, offset)
    want = torch.full((N, math.prod(shape)), float("nan"))
    want[:, start_map(ref, shape)] = drawn.cpu().flatten(1)
    assert not want.isnan().any()
    assert torch.equal(z.cpu().flatten(1), want), f"{what}: z_out differs from the generator's values at the start positions"
    assert float(z.abs().max()) <= T


def check_values(what, x, z, low, ref, bound):
    """every sample against the float64 inverse chain on the kernel's own z; low: [N,...] or [B,C,H,W] (shared)"""
    worst = 0.0
    for n in range(x.shape[0]):
        lo = low if low.dim() == 4 else low[n]
        want = R.chain_inv(z[n].cpu(), lo, ref)
        M = CR.chain_magnitude(ref, z=z[n].cpu(), low=lo, inverse=True)
        worst = max(worst, float(((x[n].cpu().double() - want).abs() / M).max()))
    print(f"[sampler] {what}: e = {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound, f"{what}: e = {worst:.3e} > {bound:.3e}"
    return worst


# ------------------------------------------------------------------------------------------------ the generator
def _raw_rand(fn, out, N, n, ss, *args):
    from cwfa_amd import _lib
    from cwfa_amd.ops import _stream
    _lib.check(fn(C.c_void_p(out.data_ptr()), N, n, ss, *args, _stream()), "rand")


@pytest.mark.parametrize("n,shift,ss", [(1003, 1, 1003), (1003, 0, 1004), (1024, 0, 1024), (3, 3, 5)])
def test_uniform_bits(n, shift, ss):
    """n not a multiple of 4, a pointer off the 16-byte grid, N = 3 at sample_offset = 5, stream 2, a seed above 2^32; a sample stride
    wider than a sample (the gaps stay untouched); the 16-byte stores (aligned, stride a multiple of four) with and without a tail."""
    from cwfa_amd import _lib, ops
    N, off, stream = 3, 5, 2
    buf = torch.full((shift + N * ss + 4,), -7.0, device="cuda")
    out = buf[shift:shift + N * ss]
    assert out.data_ptr() % 16 == 4 * shift % 16
    _raw_rand(_lib.lib().cwfa_rand_uniform_f32, out, N, n, ss, SEED, stream, off)
    got = out.view(N, ss).cpu().numpy()
    want = S.uniform(N, n, SEED, stream, off)
    assert np.array_equal(got[:, :n].view(np.uint32), want.view(np.uint32))
    assert (got[:, n:] == -7.0).all() and (buf[:shift] == -7.0).all() and (buf[shift + N * ss:] == -7.0).all()
    if ss == n:
        assert torch.equal(ops.rand_uniform((N, n), SEED, stream, off), out.view(N, n))
    # sample n of this call is sample 0 of the call at sample_offset + n; another stream differs
    assert torch.equal(ops.rand_uniform((1, n), SEED, stream, off + 2)[0], out.view(N, ss)[2, :n])
    assert not torch.equal(ops.rand_uniform((1, n), SEED, stream + 1, off + 2)[0], out.view(N, ss)[2, :n])


@pytest.mark.parametrize("T", [0.5, 1.0, 3.0, math.inf])
def test_trunc_normal(T):
    from cwfa_amd import _lib, ops
    N, n, off, stream = 3, 50001, 5, 2
    z = ops.rand_trunc_normal((N, n), T, SEED, stream, off)
    want = S.trunc_normal(N, n, T, SEED, stream, off)
    err = float(np.abs(z.cpu().numpy().astype(np.float64) - want).max())
    print(f"[sampler] truncated normal T = {T}: largest absolute error {err:.3e} (bound {NORMAL_BOUND:.3e}), largest |z| {float(z.abs().max()):.4f}")
    assert err <= NORMAL_BOUND
    assert float(z.abs().max()) <= T and float(z.abs().max()) < 5.3
    # off the 16-byte grid: the same bits
    buf = torch.empty(N * n + 4, device="cuda")
    _raw_rand(_lib.lib().cwfa_rand_trunc_normal_f32, buf[1:], N, n, n, float(T), SEED, stream, off)
    assert torch.equal(buf[1:1 + N * n].view(N, n), z)


# ------------------------------------------------------------------------------------------------ the sampler's two forms
@pytest.mark.parametrize("shared", [True, False])
def test_general_form(shared):
    """(2, 3, 5, 7): odd sizes, W < 64 -- the pull kernel; with one low for all samples and with a low per sample."""
    from cwfa_amd import ops
    shape, ref, dev, _ = case("general", 11)
    N, T = 3, 0.8
    low = lows(shape, N, 12)
    low = low[0] if shared else low
    x, z = ops.chain_inv_samples(low.cuda(), dev, N, T, SEED, stream=1, sample_offset=4, return_z=True)
    assert x.shape == (N, shape[0], 2 * shape[1]) + shape[2:] and z.shape == (N,) + shape
    check_z("general", z, ref, shape, T, SEED, 1, 4)
    check_values(f"general shared={shared}", x, z, low, ref, BOUNDS["general"])
    assert torch.equal(ops.chain_inv_samples(low.cuda(), dev, N, T, SEED, stream=1, sample_offset=4), x)      # z_out is optional


@pytest.mark.parametrize("shared", [True, False])
def test_rows4_form_with_and_without_tables(shared):
    """(2, 3, 24, 64): 16 rows per block, so the second block is half dead; two column gathers (both exchange buffers), a row and
    two channel gathers; composed tables or the dependent walk: bitwise the same."""
    from cwfa_amd import ops
    shape, ref, dev, perms = case("rows4", 13)
    N, T = 3, 1.0
    low = lows(shape, N, 14)
    low = low[0] if shared else low
    x, z = ops.chain_inv_samples(low.cuda(), dev, N, T, SEED, return_z=True)
    tabs = ops.chain_tables(perms, None, *shape[1:], "cuda")
    xt, zt = ops.chain_inv_samples(low.cuda(), dev, N, T, SEED, tables=tabs, return_z=True)
    assert torch.equal(x, xt) and torch.equal(z, zt)
    check_z("rows4", z, ref, shape, T, SEED, 0, 0)
    check_values(f"rows4 shared={shared}", x, z, low, ref, BOUNDS["rows4"])
    # ops.chain_inv on the returned latents is the same sample, to the two evaluations' rounding
    lo0 = low if shared else low[1]
    again = ops.chain_inv(z[1], lo0.cuda(), dev)
    M = CR.chain_magnitude(ref, z=z[1].cpu(), low=lo0, inverse=True)
    assert float(((again.cpu().double() - x[1].cpu().double()).abs() / M).max()) <= 2 * BOUNDS["rows4"]


def test_several_waves_per_row():
    """(1, 2, 3, 1024) with three column gathers: a row spans four waves, so a single exchange buffer (or a missing barrier) shows."""
    from cwfa_amd import ops
    shape, ref, dev, _ = case("waves", 15)
    low = lows(shape, 2, 16)
    x, z = ops.chain_inv_samples(low.cuda(), dev, 2, 1.0, 21, return_z=True)
    check_z("waves", z, ref, shape, 1.0, 21, 0, 0)
    check_values("waves", x, z, low, ref, BOUNDS["waves"])


def test_more_than_six_stages():
    from cwfa_amd import ops
    shape, ref, dev, perms = case("seven", 17)
    low = lows(shape, 2, 18)
    x, z = ops.chain_inv_samples(low.cuda(), dev, 2, math.inf, 22, return_z=True)
    check_z("seven", z, ref, shape, math.inf, 22, 0, 0)
    check_values("seven stages", x, z, low, ref, BOUNDS["seven"])
    xt = ops.chain_inv_samples(low.cuda(), dev, 2, math.inf, 22, tables=ops.chain_tables(perms, None, *shape[1:], "cuda"))
    assert torch.equal(x, xt)


@pytest.mark.parametrize("name", ["kinds_general", "kinds_rows4"])
def test_stage_kinds(name):
    """NONE / ATAN / TANH / SIGMOID with pre_scale = 0.1, a stage without s and one without t, in both forms."""
    from cwfa_amd import ops
    shape, ref, dev, _ = case(name, 19)
    low = lows(shape, 2, 20)
    x, z = ops.chain_inv_samples(low.cuda(), dev, 2, 0.5, 23, return_z=True)
    check_z(name, z, ref, shape, 0.5, 23, 0, 0)
    check_values(name, x, z, low, ref, BOUNDS[name])


def test_general_against_rows4_form():
    """The (2, 3, 24, 64) case through a low shifted by one float (not on the 16-byte grid) falls to the general form: the latents
    are bit-equal, the values within the bound of each other (and each within it of the reference)."""
    from cwfa_amd import ops
    shape, ref, dev, _ = case("rows4", 13)
    n = math.prod(shape)
    low = lows(shape, 1, 24)[0]
    buf = torch.empty(n + 4, device="cuda")
    shifted = buf[1:n + 1].view(shape)
    shifted.copy_(low)
    assert shifted.data_ptr() % 16 == 4
    xa, za = ops.chain_inv_samples(low.cuda(), dev, 3, 1.0, SEED, return_z=True)
    xg, zg = ops.chain_inv_samples(shifted, dev, 3, 1.0, SEED, return_z=True)
    assert torch.equal(za, zg)
    check_values("aligned run", xa, za, low, ref, BOUNDS["rows4"])
    check_values("shifted run (general form)", xg, zg, low, ref, BOUNDS["rows4"])
    worst = max(float(((xg[i].cpu().double() - xa[i].cpu().double()).abs() / CR.chain_magnitude(ref, z=za[i].cpu(), low=low, inverse=True)).max())
                for i in range(3))
    print(f"[sampler] general vs 16-byte form: e = {worst:.3e} (bound {BOUNDS['rows4']:.3e})")
    assert worst <= BOUNDS["rows4"]


@pytest.mark.parametrize("name", ["general", "rows4"])
def test_chunked_calls_agree(name):
    """N = 5 in one call against N = 2 plus N = 3 at sample_offset = 2: bit-equal volumes and latents."""
    from cwfa_amd import ops
    shape, ref, dev, _ = case(name, 25)
    low = lows(shape, 5, 26).cuda()
    x, z = ops.chain_inv_samples(low, dev, 5, 1.0, SEED, stream=3, sample_offset=7, return_z=True)
    xa, za = ops.chain_inv_samples(low[:2], dev, 2, 1.0, SEED, stream=3, sample_offset=7, return_z=True)
    xb, zb = ops.chain_inv_samples(low[2:], dev, 3, 1.0, SEED, stream=3, sample_offset=9, return_z=True)
    assert torch.equal(x, torch.cat([xa, xb])) and torch.equal(z, torch.cat([za, zb]))
    assert not torch.equal(ops.chain_inv_samples(low, dev, 5, 1.0, SEED, stream=4, sample_offset=7), x)


@pytest.mark.parametrize("name", ["general", "rows4"])
def test_sample_stride_beyond_2_31(name):
    """x with a sample stride of 2^31 + 16 floats in an uninitialised allocation, canaries in front of and behind sample 0: the second
    sample lands at the far end, bit-equal to the packed run, and the canaries are untouched."""
    from cwfa_amd import _lib, ops
    from cwfa_amd.ops import _chain, _stream
    shape, ref, dev, _ = case(name, 27)
    B, Cc, H, W = shape
    n = Cc * H * W
    low = lows(shape, 2, 28).cuda()
    want = ops.chain_inv_samples(low, dev, 2, 1.0, SEED, stream=1)
    x_ss = 2 ** 31 + 16
    big = torch.empty(16 + x_ss + 2 * B * n, device="cuda")
    big[:16] = -3.0
    big[16 + 2 * B * n:32 + 2 * B * n] = -3.0
    ch, keep = _chain(dev)
    x = big[16:]
    assert x.data_ptr() % 16 == 0
    _lib.check(_lib.lib().cwfa_chain_inv_samples_f32(C.c_void_p(low.data_ptr()), C.c_void_p(x.data_ptr()), None, C.byref(ch), 2, B, Cc, H, W,
                                                     B * n, n, x_ss, 2 * n, 0, 0, 1.0, C.c_uint64(SEED), 1, 0, _stream()), "chain_inv_samples")
    torch.cuda.synchronize()
    assert torch.equal(x[:2 * B * n].view(want[0].shape), want[0])
    assert torch.equal(x[x_ss:x_ss + 2 * B * n].view(want[1].shape), want[1])
    assert (big[:16] == -3.0).all() and (big[16 + 2 * B * n:32 + 2 * B * n] == -3.0).all()


def test_errors():
    from cwfa_amd import ops
    from cwfa_amd._lib import CwfaHipError
    shape, ref, dev, _ = case("general", 29)
    low = lows(shape, 2, 30).cuda()
    with pytest.raises(ValueError, match="temperature"):
        ops.chain_inv_samples(low, dev, 2, 0.0, 1)
    with pytest.raises(ValueError, match="n_samples = 3"):
        ops.chain_inv_samples(low, dev, 3, 1.0, 1)
    with pytest.raises(CwfaHipError, match="temperature"):
        ops.rand_trunc_normal((2, 8), -1.0, 1)
    with pytest.raises(CwfaHipError, match="GIN"):
        ops.chain_inv_samples(low[0], [ops.stage(torch.randn(shape).cuda(), None, gin=True)], 2, 1.0, 1)
    assert ops.rand_uniform((0, 8), 1).shape == (0, 8) and ops.rand_trunc_normal((2, 0), 1.0, 1).shape == (2, 0)


# ------------------------------------------------------------------------------------------------ statistics
def test_samples_agree_with_closed_form():
    """One step at (1, 3, 24, 64), T = 1, S = 256 samples of ONE launch at seed 87, stream 0.  r = mean over the N = 2*3*24*64 voxels
    of (sample variance / ops.chain_inv_var).  The bound is that of tests/test_gpu_posterior.py::test_samples_agree_with_closed_form:
    sd(r) <= sqrt(4 / ((S - 1) N)), |r - 1| <= 6 sd(r) = 7.8e-3, and the largest z-score of the sample means below 6.  Every voxel is
    affine in ONE latent, so its ratio is var_sample(z_e) / z_var of the element e it received, and r and the z-scores are those of
    the generator's restatement up to rounding (tests/test_sampler_cpu.py: 1.000778 and 3.60) for ANY one-to-one assignment of
    elements to positions: r is asserted against the restatement's to 1e-4 as well, which shows that every element of the block of
    samples is used exactly once with the right scale -- a latent used twice or dropped moves r.  WHICH position an element goes to
    is pinned elsewhere: by check_z (z_out bit-equal to the generator's values at the start positions) and the float64 value checks."""
    from cwfa_amd import CWFA, ops
    shape, Sn = (1, 3, 24, 64), 256
    ref, dev, _ = make_chain(shape, [None, 3, 1, 2, 3, 1], 85)
    low = torch.randn(shape, generator=torch.Generator().manual_seed(86)).cuda()
    xs = ops.chain_inv_samples(low, dev, Sn, 1.0, 87, stream=0).double()
    zv = CWFA.truncated_normal_variance(1)
    closed = ops.chain_inv_var(None, dev, zv, shape=shape).double()
    mean0 = ops.chain_inv(None, low, dev).double()
    N = closed.numel()
    r = float((xs.var(dim=0, unbiased=True) / closed).mean())
    sd = math.sqrt(4.0 / ((Sn - 1) * N))
    zscore = float(((xs.mean(0) - mean0) / (closed / Sn).sqrt()).abs().max())
    zr = S.trunc_normal(Sn, math.prod(shape), 1.0, 87)
    r_ref = float((zr.var(0, ddof=1) / zv).mean())
    z_ref = float(np.abs(zr.mean(0) / math.sqrt(zv / Sn)).max())
    print(f"[sampler] samples vs closed form: r = {r:.6f} (restatement {r_ref:.6f}), |r - 1| = {abs(r - 1):.3e}, 6 sd = {6 * sd:.3e}; "
          f"largest z-score {zscore:.3f} (restatement {z_ref:.3f})")
    assert abs(r - 1.0) <= 6.0 * sd and zscore < 6.0
    assert abs(r - r_ref) <= 1e-4


# ------------------------------------------------------------------------------------------------ the pyramid
def _pyramid(block_type="CAT"):
    """The small pyramid of tests/test_gpu_posterior.py: D = 16, side 64, three levels (two flow steps), internal_chans = 8."""
    from cwfa_amd import CWFA
    torch.manual_seed(0)
    np.random.seed(0)
    D, side, S_ = 16, 64, 3
    conv_inn, cond_nets = CWFA.build_networks(D, side, S_, block_type=block_type, internal_chans=8, cond_chans=4, with_lrnn=False)
    g = torch.Generator().manual_seed(1)
    cond_input = torch.randn(1, 29, side, side, generator=g).cuda()
    mean_cache = [(0.1 * torch.randn(1, D // 2 ** (n + 1), side, side, generator=g)).cuda() for n in range(S_ - 1)]
    low = torch.randn(1, D // 2 ** (S_ - 1), side, side, generator=g).cuda()
    return conv_inn, cond_nets, cond_input, mean_cache, low


@pytest.fixture(scope="module")
def pyramid():
    return _pyramid()


def _by_hand(conv_inn, cond_nets, cond_input, mean_cache, low, latents):
    """The reconstruction loop with given latents per step (execution order), through the graphs themselves."""
    up = low
    with torch.no_grad():
        for i, n in enumerate(range(len(conv_inn) - 1, -1, -1)):
            c = [cond_nets[n](cond_input)[-1], mean_cache[n]]
            up, _ = conv_inn[n]([latents[i], up], c=c, rev=True, jac=False)
    return up


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
def test_pyramid_seeded_samples(pyramid, n_samples):
    from cwfa_amd import CWFA
    conv_inn, cond_nets, cond_input, mean_cache, low = pyramid
    counts, undo = {}, []
    _count_calls(conv_inn, cond_nets, counts, undo)
    try:
        xs, zs = CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, n_samples, low=low, temperature=0.7, return_z=True, seed=3)
    finally:
        for u in undo:
            u()
    # every network ONCE, whatever n_samples is: 2 condition nets, 5 sub-networks per step
    assert len(counts) == 2 + 2 * 5 and all(v == 1 for v in counts.values()), counts
    assert xs.shape == (n_samples, 1, 16, 64, 64) and len(zs) == 2 and all(z.shape[0] == n_samples for z in zs)
    assert [tuple(z.shape[1:]) for z in zs] == [(1, 4, 64, 64), (1, 8, 64, 64)]
    assert all(float(z.abs().max()) <= 0.7 for z in zs)
    for i in range(n_samples):
        assert_close(xs[i], _by_hand(conv_inn, cond_nets, cond_input, mean_cache, low, [z[i] for z in zs]), TOL, f"sample {i} by hand")
    if n_samples > 1:
        assert not torch.equal(xs[0], xs[1]) and not torch.equal(zs[0][0], zs[0][1])
    # reproducible; another seed differs; sample_offset shifts the samples; without return_z the same volumes
    again = CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, n_samples, low=low, temperature=0.7, seed=3)
    assert torch.equal(again, xs)
    other = CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, n_samples, low=low, temperature=0.7, seed=4)
    assert not torch.equal(other, xs)
    last = CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, 1, low=low, temperature=0.7, seed=3, sample_offset=n_samples - 1)
    assert torch.equal(last[0], xs[n_samples - 1])
    # the two steps draw from different streams: the coarser step's latents are not a prefix of the finer step's
    assert not torch.equal(zs[0].flatten()[:64], zs[1].flatten()[:64])
    # temperature 0 is unchanged by a seed: copies of the mean
    with torch.no_grad():
        mean = CWFA.inverse_pass(conv_inn, cond_nets, cond_input, mean_cache, low=low, temperature=0)
    x0, z0 = CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, n_samples, low=low, temperature=0, return_z=True, seed=3)
    assert all(torch.equal(x0[i], mean) for i in range(n_samples)) and all(z is None for z in z0)


def test_pyramid_roi_means(pyramid):
    from cwfa_amd import CWFA, ops
    conv_inn, cond_nets, cond_input, mean_cache, low = pyramid
    boxes = np.array([[0, 16, 0, 64, 0, 64], [3, 9, 10, 20, 30, 41], [15, 16, 63, 64, 0, 1], [4, 5, 0, 64, 7, 8]], dtype=np.int32)
    counts, undo = {}, []
    _count_calls(conv_inn, cond_nets, counts, undo)
    try:
        got = CWFA.posterior_roi_means(conv_inn, cond_nets, cond_input, mean_cache, boxes, 5, low=low, temperature=0.9, seed=11, chunk=2)
    finally:
        for u in undo:
            u()
    assert all(v == 1 for v in counts.values()), counts          # three chunks, every network once
    assert got.shape == (5, 1, 4) and got.dtype == torch.float64
    xs = CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, 5, low=low, temperature=0.9, seed=11)
    want = torch.stack([ops.roi_means(xs[i], boxes).t() for i in range(5)])
    assert torch.equal(got, want)
    assert torch.equal(CWFA.posterior_roi_means(conv_inn, cond_nets, cond_input, mean_cache, boxes, 5, low=low, temperature=0.9, seed=11,
                                                chunk=16), got)
    assert float(got[:, 0, 1].std()) > 0.0
    # temperature 0: the mean's ROI means, n_samples times
    with torch.no_grad():
        mean = CWFA.inverse_pass(conv_inn, cond_nets, cond_input, mean_cache, low=low, temperature=0)
    zero = CWFA.posterior_roi_means(conv_inn, cond_nets, cond_input, mean_cache, boxes, 3, low=low, temperature=0)
    assert torch.equal(zero, ops.roi_means(mean, boxes).t().unsqueeze(0).repeat(3, 1, 1))


def test_other_block_types_raise():
    from cwfa_amd import CWFA
    conv_inn, cond_nets, cond_input, mean_cache, low = _pyramid("GLOW")
    with pytest.raises(NotImplementedError, match="affine"):
        CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, 2, low=low, seed=1)
    with pytest.raises(NotImplementedError, match="affine"):
        CWFA.posterior_roi_means(conv_inn, cond_nets, cond_input, mean_cache, np.zeros((1, 6), dtype=np.int32), 2, low=low)


def test_sample_z_truncated_with_a_seed():
    from cwfa_amd import CWFA, ops
    like = torch.empty(2, 3, 5, 7, device="cuda")
    a = CWFA.sample_z_truncated(like, device="cuda", temperature=0.7, seed=9, stream=2, sample_offset=1)
    assert torch.equal(a, ops.rand_trunc_normal((2, 3, 5, 7), 0.7, 9, 2, 1)) and float(a.abs().max()) <= 0.7
    assert torch.equal(CWFA.sample_z_truncated((2, 3, 5, 7), device="cuda", temperature=0.7, seed=9, stream=2, sample_offset=1), a)
    assert not CWFA.sample_z_truncated(like, device="cuda", temperature=0, seed=9).any()
