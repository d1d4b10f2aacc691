"""GPU (MI355X): the backward / reduction launchers of training.py and autograd.py, one by one, against a float64 restatement
of the same operation from the same fp32 inputs (upcast), at the sizes the LRNN runs (UNet(depth 3, wf 8), ConvNeXt(6,64),
ConvNeXt(64,6), GlobalAttention(6) on 512x512; the finest flow step's 48x512x512 chains) and at the edges where they go wrong.
Small edge cases take the reference from torch on the CPU; full-size ones from torch's own float64 kernels on the GPU.  Where
torch has an autograd formula (BatchNorm, LayerNorm, GELU, max-pool, PReLU, the attention's Conv1d, the affine coupling) the
reference gradient comes from float64 autograd, not from a hand-derived formula.

Tolerances:
  * Pure routing is exact.  maxpool2_bwd routes g_pool to one element of each window and adds g_skip once in fp32; the float64
    routing rounded to fp32 is that same single rounding.  scale_channels with power-of-two (or zero) factors is exact too.
    These compare with torch.equal.
  * Elementwise fp32 outputs (a few fp32 roundings per element, no reduction): assert_close (max-rel and L2-rel against the
    reference's max / norm) at 1e-6.  1e-5 where the output depends on a reduction or on fp32-rounded statistics: layernorm_bwd's
    dL/dv, dw, db; layernorm_apply (the mean is rounded to fp32 before the subtraction: ulp(3)/2 / std 0.1 = 1.2e-6 of x-hat on
    the mean-3 data); attention_bwd's gm; the BatchNorm + PReLU backward composed through the host fold.
  * Scalar and per-channel float64 sums (bn_bwd_stats, channel_stats, sample_stats, the dalpha of prelu_bwd / bn_act_bwd,
    attention_bwd's parameter gradients, chain_inv_bwd's loss sum) cancel heavily, so a bound relative to the result would be
    meaningless (the 1e-3 PReLU-slope exception of test_unet_backward_golden).  Instead, per entry,
        |got - ref| <= k * 2**-24 * sum_i |term_i|,
    |term_i| being the product of the absolute values of the term's factors (a factor that is itself a sum counts as the sum
    of the absolute values of its parts).  k = the fp32 roundings a term goes through before it reaches a double, plus the
    depth of any per-thread fp32 accumulation; the double accumulation itself adds < N * 2**-53 <= 2**-27 for N <= 2**26 terms.
    k is derived per launcher below.  Teeth: at C=256 on 512^2 losing one of the 9 splits of random data moves a channel's sum
    by ~sqrt(29000) = 170, while the k=4 bound there is ~4 * 2**-24 * 0.8 * 262144 = 0.05.
  * No bit-equality between two runs of anything reduced by float64 atomics (their order is not fixed).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

pytestmark = pytest.mark.gpu
U = 2.0 ** -24          # unit roundoff of fp32
EW = 1e-6               # elementwise outputs
RED = 1e-5              # elementwise outputs that depend on a reduction

# ------------------------------------------------------------------------------------------------ launch geometry
# Restated from the host launchers (conv_bwd.hip, lrnn_ops.hip).  Each returns (blocks along the reduced axis, cap, elements per
# thread); the module-level assertions below check that the case lists reach one block, several blocks below the cap, and exactly
# the cap with a grid-stride loop of more than one iteration.


def bn_geom(B, C, HW):          # cwfa_bn_bwd_stats_f32 / cwfa_bn_act_bwd_f32: grid (splits, C, B)
    cap = 2048 // (B * C) + 1
    splits = min(-(-HW // 4096), cap)
    return splits, cap, -(-HW // (splits * 256))


def ln_geom(n):                 # cwfa_sample_stats_f32 / ln_bwd_stats_kernel: grid (blocks, B)
    blocks = min(max(-(-n // 4096), 1), 1024)
    return blocks, 1024, -(-n // (blocks * 256))


def att_geom(L):                # cwfa_attention_bwd_f32: grid (blocks, B)
    blocks = min(-(-L // 256), 512)
    return blocks, 512, -(-L // (blocks * 256))


def prelu_geom(n):              # cwfa_prelu_bwd_f32: grid (blocks, B)
    blocks = min(-(-n // 256), 2048)
    return blocks, 2048, -(-n // (blocks * 256))


def cs_geom(B, C, HW, x_bs, offset_elems=0):     # cwfa_channel_stats_f32: grid (splits, C, B), contiguous slices per block
    splits = -(-HW // 4096)
    splits = max(min(splits, -(-4096 // (C * B))), 1)
    splits = min(splits, 64)
    vec_ok = HW % 4 == 0 and x_bs % 4 == 0 and offset_elems % 4 == 0
    per = ((-(-HW // splits)) + 3) & ~3
    return splits, 64, -(-per // 256), vec_ok


def _reach(geom, shapes):
    got = set()
    for s in shapes:
        blocks, cap, per_thread = geom(*s)[:3]
        if blocks == 1:
            got.add("one")
        elif blocks < cap:
            got.add("several")
        elif blocks == cap and per_thread > 1:
            got.add("cap")
    return got


ALL3 = {"one", "several", "cap"}

# (B, C, H, W, mask, per-sample A, PReLU slope, channel-sliced)
BN_CASES = [
    (1, 256, 512, 512, False, False, True, False),      # 9 splits (the cap), 114 elements per thread
    (1, 512, 256, 256, True, False, True, False),       # 5 splits
    (1, 1024, 128, 128, False, False, False, False),    # 3 splits
    (3, 5, 9, 11, True, True, True, True),              # HW < 256: one block per plane
    (3, 4, 37, 45, True, True, True, False),            # ragged HW
    (3, 6, 70, 90, False, True, True, True),            # 2 splits below the cap
    (2, 6, 100, 100, True, False, False, True),         # 3 splits
    (1, 7, 37, 45, False, False, True, False),          # B=1 with a [C] table
]
LN_CASES = [  # (B, C, H, W)
    (1, 64, 512, 512),          # 16.7M per sample: the 1024-block cap, 64 elements per thread
    (3, 6, 512, 512),           # 384 blocks
    (3, 5, 7, 9),               # ragged, one block
    (2, 4, 33, 31),
]
ATT_L = [1, 2, 255, 256, 257, 512 * 512]
PRELU_CASES = [(1, 6, 512, 512), (2, 8, 64, 64), (3, 1, 10, 20), (2, 5, 7, 9)]
CS_CASES = [  # (B, C, H, W, channel offset of a slice of a wider tensor, wider C)
    (1, 3, 512, 512, 0, 3), (1, 64, 512, 512, 0, 64), (2, 5, 37, 45, 1, 7), (3, 4, 9, 11, 0, 4), (1, 16, 256, 256, 1, 17),
    (2, 6, 64, 64, 2, 9)]

assert _reach(lambda B, C, H, W, *_: bn_geom(B, C, H * W), BN_CASES) == ALL3
assert _reach(lambda B, C, H, W: ln_geom(C * H * W), LN_CASES) == ALL3
assert _reach(lambda L: att_geom(L), [(L,) for L in ATT_L]) == ALL3
assert _reach(lambda B, C, H, W: prelu_geom(C * H * W), PRELU_CASES) == ALL3
assert _reach(lambda B, C, H, W, o, Cw: cs_geom(B, C, H * W, Cw * H * W, o * H * W), CS_CASES) == ALL3
assert {cs_geom(B, C, H * W, Cw * H * W, o * H * W)[3] for B, C, H, W, o, Cw in CS_CASES} == {True, False}
# the full-size split counts the LRNN's UNet takes (9, 5 and 3 splits)
assert [bn_geom(1, c, hw)[0] for c, hw in ((256, 512 * 512), (512, 256 * 256), (1024, 128 * 128))] == [9, 5, 3]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def _gen(seed, dev="cuda"):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(shape, gen, dev="cuda"):
    return torch.randn(shape, generator=gen, device=dev)


def _sliced(t, lead, extra, gen):
    """t as a channel slice [:, lead:lead + C] of a wider contiguous tensor (batch stride != C*H*W when B > 1)."""
    B, Cc, H, W = t.shape
    big = _randn((B, Cc + lead + extra, H, W), gen, t.device)
    big[:, lead:lead + Cc] = t
    v = big[:, lead:lead + Cc]
    assert v.data_ptr() != big.data_ptr() and torch.equal(v, t)
    return v


def assert_sum_bound(got, ref, absterms, k, what):
    """|got - ref| <= k * 2**-24 * sum |term|, per entry."""
    got, ref, absterms = (torch.as_tensor(t).double().cpu().reshape(-1) for t in (got, ref, absterms))
    err = (got - ref).abs()
    bound = k * U * absterms
    ok = err <= bound
    worst = int(torch.argmax(err - bound))
    assert bool(ok.all()), (f"{what}: {int((~ok).sum())} of {ok.numel()} entries out of bound; worst [{worst}] |err| {float(err[worst]):.4g}"
                            f" > {float(bound[worst]):.4g} (ref {float(ref[worst]):.6g})")


# ------------------------------------------------------------------------------------------------ plane_affine
@pytest.mark.parametrize("cfg", [(2, 5, 6, 8, False, False, False), (3, 4, 5, 12, True, False, False), (3, 4, 5, 12, True, True, True),
                                 (1, 6, 20, 20, False, True, True), (2, 3, 16, 4, True, True, False), (1, 64, 512, 512, False, True, False)])
def test_plane_affine(cfg):
    """u = x * scale[(b,)c] + shift[(b,)c] (+ add): [C] and [B,C] tables, with and without `add`, channel-sliced input."""
    from cwfa_amd import ops
    B, Cc, H, W, per, add, sliced = cfg
    g = _gen(sum(cfg[:4]))
    x = _randn((B, Cc, H, W), g)
    tshape = (B, Cc) if per else (Cc,)
    sc, sh = _randn(tshape, g), _randn(tshape, g)
    a = _randn((B, Cc, H, W), g) if add else None
    xin = _sliced(x, 1, 2, g) if sliced else x
    got = ops.plane_affine(xin, sc, sh, a)
    view = (B, Cc, 1, 1) if per else (1, Cc, 1, 1)
    ref = x.double() * sc.double().view(view) + sh.double().view(view)
    if add:
        ref = ref + a.double()
    assert_close(got, ref, EW, f"plane_affine {cfg}")
    if not add:         # table-less: the skip add alone (v = up + skip)
        assert torch.equal(ops.plane_affine(xin, add=a if a is not None else x), (x.double() + x.double()).float())


def test_plane_affine_rejects_unaligned_planes_without_launching():
    from cwfa_amd import ops
    from cwfa_amd._lib import CwfaHipError
    x = torch.randn(2, 3, 5, 7, device="cuda")                     # HW = 35: not a multiple of 4 elements
    with pytest.raises(CwfaHipError, match="multiples of 4"):
        ops.plane_affine(x, torch.ones(3, device="cuda"), torch.zeros(3, device="cuda"))
    flat = torch.randn(2 * 3 * 16 + 1, device="cuda")
    xm = flat[1:].view(2, 3, 4, 4)                                  # 4-byte offset: not 16-byte aligned
    with pytest.raises(CwfaHipError, match="aligned"):
        ops.plane_affine(xm, torch.ones(3, device="cuda"), torch.zeros(3, device="cuda"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ BatchNorm backward pieces
def _bn_inputs(cfg, seed):
    B, Cc, H, W, mask, per, prelu, sliced = cfg
    g0 = _gen(seed)
    g = _randn((B, Cc, H, W), g0)
    q = _randn((B, Cc, H, W), g0)
    q[..., ::7, ::5] = 0.0                                          # exact zeros: PReLU' takes the slope branch (strict >)
    alpha = torch.tensor([0.25], device="cuda") if prelu else None
    y = torch.where(q > 0, q, (alpha if prelu else 1.0) * q)        # the conv output y = PReLU(q), fp32
    m = None
    if mask:
        keep = torch.rand((B, Cc), generator=g0, device="cuda") >= 0.3
        m = keep.float() / (1.0 - 0.3)                             # zeros and 1/(1-p)
        assert bool((m == 0).any()) and bool((m > 0).any())
    gin, yin = (_sliced(g, 2, 1, g0), _sliced(y, 1, 3, g0)) if sliced else (g, y)
    return g, y, q, m, alpha, gin, yin


@pytest.mark.parametrize("cfg", BN_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}" for c in BN_CASES])
def test_bn_bwd_stats_and_bn_act_bwd(cfg):
    """S1 = sum g*m, S2 = sum g*m*y per channel; then (A g + Bc + Cc y) * PReLU'(y) with dalpha += sum (...) * min(q, 0)."""
    from cwfa_amd import ops
    B, Cc, H, W, mask, per, prelu, sliced = cfg
    g, y, q, m, alpha, gin, yin = _bn_inputs(cfg, 1000 + sum(cfg[:4]))
    st = ops.bn_bwd_stats(gin, yin, m)
    gd, yd = g.double(), y.double()
    md = m.double().view(B, Cc, 1, 1) if m is not None else torch.ones(1, dtype=torch.float64, device="cuda")
    gm = gd * md
    # k = 4: g*m is rounded once in fp32, the product with y is exact in double, the per-thread and block sums are double
    assert_sum_bound(st[:, 0], gm.sum((0, 2, 3)), gm.abs().sum((0, 2, 3)), 4, f"S1 {cfg}")
    assert_sum_bound(st[:, 1], (gm * yd).sum((0, 2, 3)), (gm * yd).abs().sum((0, 2, 3)), 4, f"S2 {cfg}")
    del gm
    g1 = _gen(7 + Cc)
    A = _randn((B, Cc) if per else (Cc,), g1)
    Bc, Cf = _randn((Cc,), g1), _randn((Cc,), g1)
    base = 0.37
    dalpha = torch.full((1,), base, dtype=torch.float64, device="cuda") if prelu else None
    out = ops.bn_act_bwd(gin, yin, A, Bc, Cf, alpha, dalpha)
    Ad = A.double().view(B, Cc, 1, 1) if per else A.double().view(1, Cc, 1, 1)
    bcd, ccd = Bc.double().view(1, Cc, 1, 1), Cf.double().view(1, Cc, 1, 1)
    gy = Ad * gd + bcd + ccd * yd
    if prelu:
        pos = y > 0
        ref = torch.where(pos, gy, float(alpha) * gy)
        qd = yd / float(alpha)
        # k = 4: gy = a*g + bc + cc*y takes three fp32 roundings (the products and two adds), counted against
        # |a g| + |bc| + |cc y|; the product with q = y / alpha is formed in double
        terms = torch.where(pos, torch.zeros_like(qd), (Ad * gd).abs() + bcd.abs() + (ccd * yd).abs()) * qd.abs()
        assert_sum_bound(dalpha - base, torch.where(pos, torch.zeros_like(qd), gy * qd).sum(), terms.sum(), 4, f"dalpha {cfg}")
        del terms, qd
    else:
        ref = gy
    assert_close(out, ref, EW, f"bn_act_bwd {cfg}")


@pytest.mark.parametrize("cfg", [(3, 8, 64, 64, True, True, True, False), (1, 16, 128, 128, False, False, True, True),
                                 (2, 6, 37, 45, True, True, True, True)])
def test_batchnorm_prelu_backward_vs_autograd(cfg):
    """The two launchers composed as training._block_backward composes them (the host fold of S1, S2, the batch statistics and
    gamma into A, Bc, Cc), against float64 autograd of  u = BatchNorm_train(PReLU(q)) * mask."""
    from cwfa_amd import ops
    B, Cc, H, W, mask, per, prelu, sliced = cfg
    g, y, q, m, alpha, gin, yin = _bn_inputs(cfg, 2000 + sum(cfg[:4]))
    gw = _gen(5)
    w = 1.0 + 0.3 * _randn((Cc,), gw)
    bia = 0.1 * _randn((Cc,), gw)
    q64 = torch.where(y > 0, y.double(), y.double() / float(alpha)).requires_grad_()
    a64 = alpha.double().requires_grad_()
    w64, b64 = w.double().requires_grad_(), bia.double().requires_grad_()
    u = F.batch_norm(F.prelu(q64, a64), None, None, w64, b64, True, 0.0, 1e-5)
    if m is not None:
        u = u * m.double().view(B, Cc, 1, 1)
    u.backward(g.double())
    n = B * H * W
    yd = y.double()
    mean = yd.mean((0, 2, 3))
    invstd = torch.rsqrt(yd.var((0, 2, 3), unbiased=False) + 1e-5)
    st = ops.bn_bwd_stats(gin, yin, m)
    s1, s2 = st[:, 0], st[:, 1]
    s2h = (s2 - mean * s1) * invstd
    k = w.double() * invstd
    A = k if m is None else m.double() * k[None, :]
    Cf = -k * invstd * s2h / n
    Bc = -k * s1 / n - Cf * mean
    dalpha = torch.zeros(1, dtype=torch.float64, device="cuda")
    gq = ops.bn_act_bwd(gin, yin, A.float(), Bc.float(), Cf.float(), alpha, dalpha)
    assert_close(gq, q64.grad, RED, f"dL/dq {cfg}")
    assert_close(s2h, w64.grad, RED, f"dL/dgamma {cfg}")
    assert_close(s1, b64.grad, RED, f"dL/dbeta {cfg}")
    assert abs(float(dalpha) - float(a64.grad)) <= RED * float((q64.grad.abs() * torch.clamp(q64.detach(), max=0).abs()).sum() / float(alpha))


# ------------------------------------------------------------------------------------------------ max-pool backward
def _pool_ref(full64, gp64, gs64):
    _, idx = F.max_pool2d(full64, 2, return_indices=True)
    B, Cc, H, W = full64.shape
    out = torch.zeros(B, Cc, H * W, dtype=torch.float64, device=full64.device)
    out.scatter_(2, idx.view(B, Cc, -1), gp64.view(B, Cc, -1))
    out = out.view(B, Cc, H, W)
    return out if gs64 is None else out + gs64


@pytest.mark.parametrize("skip", [False, True])
def test_maxpool2_bwd_ties_signed_zeros_and_nan(skip):
    """Windows with ties (inputs quantised to {-1, 0, 1}: the first maximum in window order wins), +-0 ties (equal: the first
    wins), NaN (wins over anything; the last NaN of a window wins) -- the reference is ATen's own max-pool index rule, float64 on
    the CPU.  g_skip is added with one fp32 add, so the result is exact."""
    from cwfa_amd import ops
    g0 = torch.Generator().manual_seed(31)
    B, Cc, H, W = 2, 3, 10, 14
    full = torch.randint(-1, 2, (B, Cc, H, W), generator=g0).float()
    full[0, 0, 0, :4] = torch.tensor([0.0, -0.0, -0.0, 0.0])
    full[0, 0, 1, :4] = torch.tensor([-0.0, 0.0, 0.0, -0.0])
    full[0, 1, :2, :2] = torch.tensor([[1.0, float("nan")], [float("nan"), 1.0]])       # two NaNs: the last one wins
    full[1, 2, 2:4, 2:4] = torch.tensor([[float("nan"), 5.0], [1.0, float("nan")]])
    full[1, 0, 4:6, 6:8] = torch.tensor([[-1.0, float("nan")], [1.0, 2.0]])
    full[1, 1, 6:8, 0:2] = float("-inf")
    gp = torch.randn(B, Cc, H // 2, W // 2, generator=g0)
    gs = torch.randn(B, Cc, H, W, generator=g0) if skip else None
    ref = _pool_ref(full.double(), gp.double(), None if gs is None else gs.double()).float()
    got = ops.maxpool2_bwd(full.cuda(), gp.cuda(), None if gs is None else gs.cuda()).cpu()
    assert torch.equal(got, ref), (got - ref).abs().max()


@pytest.mark.parametrize("shape", [(1, 256, 512, 512), (1, 1024, 128, 128), (2, 8, 6, 10)])
def test_maxpool2_bwd_full_size(shape):
    from cwfa_amd import ops
    g0 = _gen(sum(shape))
    B, Cc, H, W = shape
    full = _randn(shape, g0)
    full[..., ::3, ::2] = torch.round(full[..., ::3, ::2])
    gp = _randn((B, Cc, H // 2, W // 2), g0)
    gs = _randn(shape, g0)
    for skip in (None, gs):
        ref = _pool_ref(full.double(), gp.double(), None if skip is None else skip.double()).float()
        assert torch.equal(ops.maxpool2_bwd(full, gp, skip), ref), shape


def test_maxpool2_bwd_grid_limits():
    """B*C = 65535 planes run (grid y); 65536 and odd H / W are rejected before a launch."""
    from cwfa_amd import ops
    from cwfa_amd._lib import CwfaHipError
    g0 = _gen(9)
    full = _randn((1, 65535, 2, 2), g0)
    gp = _randn((1, 65535, 1, 1), g0)
    assert torch.equal(ops.maxpool2_bwd(full, gp), _pool_ref(full.double(), gp.double(), None).float())
    with pytest.raises(CwfaHipError, match="B\\*C"):
        ops.maxpool2_bwd(torch.zeros(2, 32768, 2, 2, device="cuda"), torch.zeros(2, 32768, 1, 1, device="cuda"))
    with pytest.raises(CwfaHipError, match="even"):
        ops.maxpool2_bwd(torch.zeros(1, 2, 5, 4, device="cuda"), torch.zeros(1, 2, 2, 2, device="cuda"))
    with pytest.raises(CwfaHipError, match="even"):
        ops.maxpool2_bwd(torch.zeros(1, 2, 4, 7, device="cuda"), torch.zeros(1, 2, 2, 3, device="cuda"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ PReLU backward
@pytest.mark.parametrize("shape", PRELU_CASES)
def test_prelu_bwd_sizes_and_in_place(shape):
    """g * PReLU'(q) and dalpha += sum g * min(q, 0), q recovered from the output as o / alpha.  The 6x512x512 case is the UNet's
    last layer: the 2048-block cap with a 3-iteration grid-stride loop.  In place (out = g, as cond_backward calls it) equals the
    out-of-place call bit for bit."""
    from cwfa_amd import ops
    g0 = _gen(sum(shape) + 40)
    q = _randn(shape, g0)
    q[..., ::4, ::3] = 0.0
    gup = _randn(shape, g0)
    alpha = torch.tensor([0.3], device="cuda")
    o = torch.where(q > 0, q, alpha * q)
    q64 = torch.where(o > 0, o.double(), o.double() / float(alpha)).requires_grad_()
    a64 = alpha.double().requires_grad_()
    F.prelu(q64, a64).backward(gup.double())
    base = -1.25
    da = torch.full((1,), base, dtype=torch.float64, device="cuda")
    got = ops.prelu_bwd(gup, o, alpha, da)
    assert_close(got, q64.grad, EW, f"prelu_bwd {shape}")
    # k = 4: the term g * (o / alpha) is formed in double from fp32 operands (one rounding of the quotient), summed in double
    terms = (gup.double() * torch.clamp(q64.detach(), max=0)).abs().sum()
    assert_sum_bound(da - base, a64.grad, terms, 4, f"dalpha {shape}")
    da2 = torch.zeros(1, dtype=torch.float64, device="cuda")
    gi = gup.clone()
    ops.prelu_bwd(gi, o, alpha, da2, out=gi)
    assert torch.equal(gi, got), "in-place prelu_bwd differs from the out-of-place call"
    assert_sum_bound(da2, a64.grad, terms, 4, f"dalpha in place {shape}")


# ------------------------------------------------------------------------------------------------ GELU
SPECIAL_P = [0.0, 1e-3, -1e-3, 3.0, -3.0, 10.0, -10.0]


@pytest.mark.parametrize("shape", [(2, 6, 37, 45), (1, 64, 128, 128)])
def test_gelu_add_and_gelu_bwd(shape):
    """GELU(p) + res and g * GELU'(p) against F.gelu (erf form) in float64 and its autograd; p includes 0, +-1e-3, +-3, +-10."""
    from cwfa_amd import ops
    g0 = _gen(sum(shape) + 3)
    p = 2.0 * _randn(shape, g0)
    flat = p.view(-1)
    flat[:len(SPECIAL_P) * 5] = torch.tensor(SPECIAL_P * 5, device="cuda")
    res = _randn(shape, g0)
    gup = _randn(shape, g0)
    p64 = p.double().requires_grad_()
    y64 = F.gelu(p64)
    y64.backward(gup.double())
    assert_close(ops.gelu_add(p), y64.detach(), EW, "gelu")
    assert_close(ops.gelu_add(p, res), y64.detach() + res.double(), EW, "gelu + res")
    got = ops.gelu_bwd(gup, p)
    assert_close(got, p64.grad, EW, "gelu backward")
    sp = flat[:len(SPECIAL_P)]
    ref_sp = p64.grad.view(-1)[:len(SPECIAL_P)]
    assert torch.allclose(got.view(-1)[:len(SPECIAL_P)].double(), ref_sp, rtol=1e-6, atol=1e-7), (sp, got.view(-1)[:7], ref_sp)


# ------------------------------------------------------------------------------------------------ LayerNorm over (C,H,W)
def _ln_data(shape, seed, kind):
    B = shape[0]
    g0 = _gen(seed)
    if kind == "const":
        return torch.full(shape, 0.1, device="cuda")
    v = 0.1 * _randn(shape, g0) + 3.0 if kind == "mean3" else _randn(shape, g0)
    return v + torch.arange(B, device="cuda", dtype=torch.float32).view(B, 1, 1, 1) * 0.5       # samples differ in mean


@pytest.mark.parametrize("shape", LN_CASES)
@pytest.mark.parametrize("kind", ["plain", "mean3"])
def test_sample_stats_layernorm_apply_and_bwd(shape, kind):
    """sample_stats (per-sample sum / sum of squares), layernorm_apply, layernorm_bwd (dL/dv; dw, db added into existing non-zero
    gradients) against float64 F.layer_norm and its autograd.  Mean-3 / std-0.1 data stresses E[x^2] - E[x]^2."""
    from cwfa_amd import ops
    B = shape[0]
    n = math.prod(shape[1:])
    v = _ln_data(shape, sum(shape), kind)
    gw = _gen(77)
    w = 1.0 + 0.5 * _randn(shape[1:], gw)
    bia = 0.3 * _randn(shape[1:], gw)
    st = ops.sample_stats(v).view(B, 2)
    vd = v.double().view(B, -1)
    # k = 4: every term (x and x*x of an fp32 x) is exact in double; only the double accumulation rounds
    assert_sum_bound(st[:, 0], vd.sum(1), vd.abs().sum(1), 4, f"sum x {shape}")
    assert_sum_bound(st[:, 1], (vd * vd).sum(1), (vd * vd).sum(1), 4, f"sum x^2 {shape}")
    del vd
    v64 = v.double().requires_grad_()
    w64, b64 = w.double().requires_grad_(), bia.double().requires_grad_()
    y64 = F.layer_norm(v64, shape[1:], w64, b64, 1e-5)
    assert_close(ops.layernorm_apply(v, st.reshape(-1), w, bia, 1e-5), y64.detach(), RED, f"layernorm_apply {shape} {kind}")
    gup = _randn(shape, _gen(5 + B)) + 0.5 * y64.detach().float()          # correlated with x-hat: S2 is not small
    y64.backward(gup.double())
    mean = st[:, 0] / n
    invstd = torch.rsqrt(st[:, 1] / n - mean * mean + 1e-5)
    dw0, db0 = _randn(shape[1:], gw), _randn(shape[1:], gw)
    dw, db = dw0.clone(), db0.clone()
    gv = ops.layernorm_bwd(gup, v, w, mean.float(), invstd.float(), dw, db)
    assert_close(gv, v64.grad, RED, f"dL/dv {shape} {kind}")
    assert_close(dw, w64.grad + dw0.double(), RED, f"dw {shape} {kind}")
    assert_close(db, b64.grad + db0.double(), RED, f"db {shape} {kind}")


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (1, 6, 512, 512)])
def test_layernorm_apply_of_a_constant_plane_is_the_bias(shape):
    """Variance 0 (clamped at 0 when E[x^2] - E[x]^2 rounds below it): x - mean = 0 exactly, the output is the bias."""
    from cwfa_amd import ops
    v = _ln_data(shape, 1, "const")
    bia = _randn(shape[1:], _gen(2))
    w = _randn(shape[1:], _gen(3))
    st = ops.sample_stats(v)
    got = ops.layernorm_apply(v, st, w, bia, 1e-5)
    assert torch.equal(got, bia.expand(shape))
    assert_close(got, F.layer_norm(v.double(), shape[1:], w.double(), bia.double(), 1e-5), EW, "constant plane")


# ------------------------------------------------------------------------------------------------ channel_stats
@pytest.mark.parametrize("cfg", CS_CASES)
def test_channel_stats(cfg):
    """(sum, sum of squares) per channel over (B,H,W): the vectorised and scalar slice loops, channel-sliced inputs."""
    from cwfa_amd import ops
    B, Cc, H, W, lead, Cw = cfg
    g0 = _gen(sum(cfg))
    x = _randn((B, Cc, H, W), g0) + 2.0
    xin = _sliced(x, lead, Cw - Cc - lead, g0) if Cw != Cc else x
    st = ops.channel_stats(xin).view(Cc, 2)
    xd = x.double()
    # k = 4: the terms are exact in double (fp32 x, x*x formed in double); only the double accumulation rounds
    assert_sum_bound(st[:, 0], xd.sum((0, 2, 3)), xd.abs().sum((0, 2, 3)), 4, f"sum {cfg}")
    assert_sum_bound(st[:, 1], (xd * xd).sum((0, 2, 3)), (xd * xd).sum((0, 2, 3)), 4, f"sumsq {cfg}")


# ------------------------------------------------------------------------------------------------ attention
def _att_ref(mean, w1, b1, w2, b2):
    """GlobalAttention's sigmoid(Conv1d_k1(relu(Conv1d_k3(s, padding 1)))) along the flattened H*W sequence; returns (att, h, a)."""
    B, Cc = mean.shape[:2]
    s = mean.reshape(B, Cc, -1)
    L = s.shape[2]
    sp = F.pad(s, (1, 1))
    h = b1.view(1, -1, 1) + sum(torch.einsum("oc,bcl->bol", w1[:, :, k], sp[:, :, k:k + L]) for k in range(3))
    a = b2.view(1, -1, 1) + torch.einsum("oc,bcl->bol", w2[:, :, 0], torch.relu(h))
    return torch.sigmoid(a), h, a


def _att_params(Cc, seed):
    g0 = _gen(seed)
    r1, r2 = 1.0 / math.sqrt(3 * Cc), 1.0 / math.sqrt(Cc)          # nn.Conv1d's default init ranges
    w1 = (2 * torch.rand((Cc, Cc, 3), generator=g0, device="cuda") - 1) * r1
    b1 = (2 * torch.rand((Cc,), generator=g0, device="cuda") - 1) * r1
    w2 = (2 * torch.rand((Cc, Cc, 1), generator=g0, device="cuda") - 1) * r2
    b2 = (2 * torch.rand((Cc,), generator=g0, device="cuda") - 1) * r2
    return w1, b1, w2, b2


def _att_shape(B, Cc, L):
    return (B, Cc, 512, 512) if L == 512 * 512 else (B, Cc, 1, L)


@pytest.mark.parametrize("Cc", [1, 6, 8, 16])
@pytest.mark.parametrize("L", ATT_L)
def test_attention_combine(Cc, L):
    """out = x + 2 m (att - 0.5) (m given), 2 m (att - 0.5) (x None), att (m None); B = 2 (the i +- 1 neighbours stop at each
    sample's sequence ends, not at block edges)."""
    from cwfa_amd import ops
    B = 2
    shape = _att_shape(B, Cc, L)
    g0 = _gen(Cc * 1000 + L)
    mean, m, x = _randn(shape, g0), _randn(shape, g0), _randn(shape, g0)
    w1, b1, w2, b2 = _att_params(Cc, Cc)
    att = _att_ref(mean.double(), w1.double(), b1.double(), w2.double(), b2.double())[0].view(shape)
    core = 2.0 * m.double() * (att - 0.5)
    assert_close(ops.attention_combine(mean, w1, b1, w2, b2, m, x), x.double() + core, EW, f"combine C={Cc} L={L}")
    # without x the output is 2 m (att - 0.5) alone: att - 0.5 cancels and the fp32 att carries an error of ulp(0.5), so the scale
    # of this output's error is max |2 m|, not max |2 m (att - 0.5)|
    err = float((ops.attention_combine(mean, w1, b1, w2, b2, m, None).double() - core).abs().max())
    assert err <= EW * float(2.0 * m.abs().max()), f"combine x=None C={Cc} L={L}: {err:.3e}"
    assert_close(ops.attention_combine(mean, w1, b1, w2, b2), att, EW, f"attention C={Cc} L={L}")


@pytest.mark.parametrize("Cc", [1, 6, 8])
@pytest.mark.parametrize("L", ATT_L)
def test_attention_bwd(Cc, L):
    """gm = dL/dm and the float64 [w1 | b1 | w2 | b2] gradients of out = x + 2 m (att - 0.5), against float64 autograd; the
    sequence is cut into blocks of 256 positions (and at most 512 blocks), so the i +- 1 neighbours cross block edges."""
    from cwfa_amd import ops
    B = 2
    shape = _att_shape(B, Cc, L)
    g0 = _gen(Cc * 7000 + L)
    mean, m, gup = _randn(shape, g0), _randn(shape, g0), _randn(shape, g0)
    w1, b1, w2, b2 = _att_params(Cc, 10 + Cc)
    leaves = [t.double().requires_grad_() for t in (w1, b1, w2, b2)]
    m64 = m.double().requires_grad_()
    att, h, a = _att_ref(mean.double(), *leaves)
    out = 2.0 * m64 * (att.view(shape) - 0.5)
    out.backward(gup.double())
    gm, pg = ops.attention_bwd(mean, w1, b1, w2, b2, m, gup)
    assert_close(gm, m64.grad, RED, f"gm C={Cc} L={L}")
    ref = torch.cat([t.grad.reshape(-1) for t in leaves])
    # |term|: the hidden unit h = b1 + sum_{c,k} w1 nb (3C fma) counts as H = |b1| + sum |w1| |nb|, the logit a = b2 + sum w2 relu(h)
    # as A = |b2| + sum |w2| H; the per-position gradient ga = 2 g m att (1 - att) carries a relative error of the logit's
    # absolute one, so ga counts as |ga| (1 + A).  k = 4C + 16: 3C + 1 roundings of h, C + 1 of a, ~4 in expf and the sigmoid,
    # 4 in ga, 2 in gh = relu'(h) sum w2 ga, 2 for the per-thread fp32 partial sums (<= 2 iterations) and the products.
    s = mean.double().reshape(B, Cc, -1)
    sp = F.pad(s.abs(), (1, 1))
    Lq = s.shape[2]
    nb = [sp[:, :, k:k + Lq] for k in range(3)]
    Ha = b1.double().abs().view(1, -1, 1) + sum(torch.einsum("oc,bcl->bol", w1.double()[:, :, k].abs(), nb[k]) for k in range(3))
    hid_a = torch.where(h.detach() > 0, Ha, torch.zeros_like(Ha))
    Aa = b2.double().abs().view(1, -1, 1) + torch.einsum("oc,bcl->bol", w2.double()[:, :, 0].abs(), hid_a)
    att_d = att.detach()
    ga = (2.0 * gup.double().reshape(B, Cc, -1) * m.double().reshape(B, Cc, -1) * att_d * (1 - att_d)).abs() * (1.0 + Aa)
    gh = torch.einsum("oc,bol->bcl", w2.double()[:, :, 0].abs(), ga)
    # a ReLU whose input lies within the fp32 error of h may switch either way: its position's terms enter the bound whole
    amb = (h.detach().abs() <= (3 * Cc + 8) * U * Ha).double()
    gh_b = gh * ((h.detach() > 0).double() + amb * (2.0 ** 24) / (4 * Cc + 16))
    t_w1 = torch.stack([torch.einsum("bol,bcl->oc", gh_b, nb[k]) for k in range(3)], 2)
    t_b1 = gh_b.sum((0, 2))
    t_w2 = torch.einsum("bol,bcl->oc", ga, Ha * ((h.detach() > 0).double() + amb * (2.0 ** 24) / (4 * Cc + 16)))
    t_b2 = ga.sum((0, 2))
    terms = torch.cat([t_w1.reshape(-1), t_b1, t_w2.reshape(-1), t_b2])
    assert_sum_bound(pg, ref, terms, 4 * Cc + 16, f"parameter gradients C={Cc} L={L}")


def test_attention_channel_limits():
    """The forward builds up to 16 channels, the backward 8 (its per-thread partial sums): C=17 / C=9 are refused cleanly.  The
    mismatch is deliberate (the LRNN has C = 6) and pinned here, so that raising either limit is a visible change."""
    from cwfa_amd import ops
    from cwfa_amd._lib import CwfaHipError
    for Cc, fn in ((17, "combine"), (9, "bwd")):
        t = torch.zeros(1, Cc, 4, 4, device="cuda")
        w1, b1, w2, b2 = _att_params(Cc, 1)
        with pytest.raises(CwfaHipError, match=f"C={Cc} not in 1..{16 if fn == 'combine' else 8}"):
            if fn == "combine":
                ops.attention_combine(t, w1, b1, w2, b2, t, t)
            else:
                ops.attention_bwd(t, w1, b1, w2, b2, t, t)
    t = torch.zeros(1, 9, 4, 4, device="cuda")
    ops.attention_combine(t, *_att_params(9, 1), t, t)              # 9 channels: forward yes, backward no
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ scale_channels / axpby
@pytest.mark.parametrize("shape", [(2, 64, 512, 512), (3, 5, 7, 9), (1, 1, 1, 1)])
def test_scale_channels_and_axpby(shape):
    """The drop-path gate (factors 0 and 1/keep; with power-of-two factors exact) and the residual gradient a x + b z."""
    from cwfa_amd import ops
    B, Cc = shape[:2]
    g0 = _gen(sum(shape) + 11)
    x, z = _randn(shape, g0), _randn(shape, g0)
    p2 = torch.tensor([0.0, 0.5, 1.0, 2.0, 4.0, -0.25], device="cuda")
    sc = p2[torch.randint(0, 6, (B, Cc), generator=g0, device="cuda")]
    assert torch.equal(ops.scale_channels(x, sc), (x.double() * sc.double().view(B, Cc, 1, 1)).float())
    sc = torch.rand((B, Cc), generator=g0, device="cuda") / 0.95
    assert_close(ops.scale_channels(x, sc), x.double() * sc.double().view(B, Cc, 1, 1), EW, "scale_channels")
    assert_close(ops.axpby(x, 1.0, z, 1.0), x.double() + z.double(), EW, "x + z")
    assert_close(ops.axpby(x, -0.7, z, 1.3), -0.7 * x.double() + 1.3 * z.double(), EW, "a x + b z")
    assert torch.equal(ops.axpby(x, 0.5), (0.5 * x.double()).float())


# ------------------------------------------------------------------------------------------------ affine stage backward
CLAMPS = {"NONE": lambda a, c: c * a, "ATAN": lambda a, c: c * 0.636 * torch.atan(a), "TANH": lambda a, c: c * torch.tanh(a),
          "SIGMOID": lambda a, c: c * 2.0 * (torch.sigmoid(a) - 0.5)}


@pytest.mark.parametrize("clamp", list(CLAMPS))
@pytest.mark.parametrize("gin", [0, 1])
@pytest.mark.parametrize("rev", [0, 1])
def test_affine_bwd(rev, gin, clamp):
    """One coupling stage y = e^s x + t (rev: (x - t) e^-s), s = clamp(pre s_raw) [GIN: minus its channel mean], t = pre t_raw,
    log-det +-sum s (GIN: 0): dL/dx, dL/ds_raw, dL/dt_raw from float64 autograd of  sum g y + sum gld logdet.  gld None / given,
    `want` subsets, channel-sliced x / g, ragged HW."""
    from cwfa_amd import ops
    for B, Cc, H, W, sliced, with_gld, want in ((2, 6, 9, 13, False, True, (True, True, True)), (3, 4, 37, 45, True, False, (True, True, True)),
                                                (1, 5, 16, 16, True, True, (False, True, False)), (2, 3, 1, 7, False, True, (True, False, True))):
        g0 = _gen(rev * 100 + gin * 10 + len(clamp) + Cc)
        x, gup = _randn((B, Cc, H, W), g0), _randn((B, Cc, H, W), g0)
        s_raw, t_raw = _randn((B, Cc, H, W), g0), _randn((B, Cc, H, W), g0)
        gld = _randn((B,), g0) if with_gld else None
        pre, cl = 0.7, 1.5
        stg = ops.stage(s_raw, t_raw, clamp, cl, pre_scale=pre, gin=bool(gin))
        xin, gi = (_sliced(x, 1, 1, g0), _sliced(gup, 2, 0, g0)) if sliced else (x, gup)
        gx, gs, gt = ops.affine_bwd(xin, gi, stg, rev, gld, want)
        x64, s64, t64 = (t.double().requires_grad_() for t in (x, s_raw, t_raw))
        s = CLAMPS[clamp](pre * s64, cl)
        if gin:
            s = s - s.mean(1, keepdim=True)
        t = pre * t64
        y = (x64 - t) * torch.exp(-s) if rev else torch.exp(s) * x64 + t
        loss = (y * gup.double()).sum()
        if gld is not None and not gin:
            loss = loss + (gld.double() * (-1 if rev else 1) * s.flatten(1).sum(1)).sum()
        loss.backward()
        what = f"rev={rev} gin={gin} {clamp} {(B, Cc, H, W)}"
        for got, ref, on, name in ((gx, x64.grad, want[0], "dx"), (gs, s64.grad, want[1], "ds_raw"), (gt, t64.grad, want[2], "dt_raw")):
            if on:
                assert_close(got, ref, EW, f"{name} {what}")
            else:
                assert got is None


# ------------------------------------------------------------------------------------------------ inverse chain backward
def _st64(st):
    s = CLAMPS[st["clamp"]](st["pre"] * st["s_raw"], 2.0) if st["s_raw"] is not None else 0.0
    if st["t"] is None:
        t = 0.0
    else:
        t = -st["t"] / math.sqrt(2.0) if st["neg"] else st["pre"] * st["t"]
    return s, t


def _fwd64(v, stages):
    for st in stages:
        if st["perm"] is not None:
            v = v.index_select(st["axis"], st["perm"])
        s, t = _st64(st)
        v = torch.exp(s) * v + t
    return v


def _inv64(z, low, stages):
    v = z
    for st in reversed(stages):
        s, t = _st64(st)
        v = (v - t) * torch.exp(-s)
        if st["perm"] is not None:
            v = v.index_select(st["axis"], torch.argsort(st["perm"]))
    B, Cc, H, W = low.shape
    r = 1.0 / math.sqrt(2.0)
    return torch.stack([(low + v) * r, (low - v) * r], 2).reshape(B, 2 * Cc, H, W)


def _chain_case(shape, n_stages, seed, dev):
    B, Cc, H, W = shape
    g0 = _gen(seed, dev)
    axes = [None, 1, 2, 3, 1, 3, 2, None][:n_stages]
    ref, stages, leaves = [], [], []
    for k, ax in enumerate(axes):
        s_raw, t = 0.5 * _randn(shape, g0, dev), _randn(shape, g0, dev)
        perm = None if ax is None else torch.randperm([0, Cc, H, W][ax], generator=g0, device=dev)
        sr, tr = s_raw.double().requires_grad_(), t.double().requires_grad_()
        leaves.append((sr, tr))
        clamp = ("ATAN", "TANH", "SIGMOID", "NONE")[k % 4]
        ref.append({"s_raw": sr, "t": tr, "perm": perm, "axis": ax, "clamp": clamp, "pre": 0.8, "neg": k == 0})
        stages.append(_op_stage(s_raw, t, clamp, perm, ax, k == 0))
    return ref, stages, leaves


def _op_stage(s_raw, t, clamp, perm, ax, neg):
    from cwfa_amd import ops
    return ops.stage(s_raw.cuda(), t.cuda(), clamp, 2.0, pre_scale=0.8, t_neg_div_sqrt2=neg, perm=None if perm is None else perm.cuda(),
                     axis=ax or 1)


@pytest.mark.parametrize("n_stages", [1, 8])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("shape", [(2, 6, 9, 12), (1, 5, 16, 70)])
def test_chain_inv_bwd(shape, kind, n_stages):
    """Backward of the inverse chain xhat = Haar1D^-1(cat[low, A_0^-1 .. A_{K-1}^-1(z)]) from xhat alone (the kernel re-runs the
    stages forwards from the detail band of xhat), with gathers on all three axes: ds_raw, dt_raw per stage (fresh and
    accumulated), dL/dz, dL/dlow (kind 0) against float64 autograd of the restated inverse chain.  Upstream gradient: kind 0
    gscale * gt, kind 1 gscale * sign(xhat - gt) (0 where xhat == gt exactly), kind 2 gscale * (xhat - gt)."""
    from cwfa_amd import ops
    B, Cc, H, W = shape
    ref, stages, leaves = _chain_case(shape, n_stages, sum(shape) + 13 * kind + n_stages, "cpu")
    g0 = torch.Generator().manual_seed(3 + kind)
    xhat = torch.randn(B, 2 * Cc, H, W, generator=g0)
    gt = torch.randn(B, 2 * Cc, H, W, generator=g0) if kind != 1 else xhat + torch.randn(B, 2 * Cc, H, W, generator=g0)
    if kind == 1:
        gt.view(-1)[::3] = xhat.view(-1)[::3]                     # exact ties: L1 gives gradient 0 there
    gscale = 0.37
    xd = xhat.double()
    hi = (xd[:, 0::2] - xd[:, 1::2]) / math.sqrt(2.0)
    lo = (xd[:, 0::2] + xd[:, 1::2]) / math.sqrt(2.0)
    z64 = _fwd64(hi, [{**st, "s_raw": st["s_raw"].detach(), "t": st["t"].detach()} for st in ref]).requires_grad_()
    low64 = lo.clone().requires_grad_()
    xr = _inv64(z64, low64, ref)
    assert_close(xr.detach(), xd, 1e-12, "float64 restatement round trip")
    d = xhat - gt
    G = {0: gscale * gt.double(), 1: gscale * torch.sign(d).double(), 2: gscale * d.double()}[kind]
    xr.backward(G)
    mk = lambda: [(torch.zeros(B, Cc, H, W, device="cuda"), torch.zeros(B, Cc, H, W, device="cuda")) for _ in stages]   # noqa: E731
    grads = mk()
    out = ops.chain_inv_bwd(xhat.cuda(), gt.cuda(), stages, grads, gscale, loss_kind=kind, want_latent_grad=True, want_low_grad=kind == 0)
    loss, gz, glow = out
    for k, ((ds, dt), (sr, tr)) in enumerate(zip(grads, leaves)):
        assert_close(ds, sr.grad, EW, f"ds_raw stage {k}")
        assert_close(dt, tr.grad, EW, f"dt_raw stage {k}")
    assert_close(gz, z64.grad, EW, "dL/dz")
    if kind == 0:
        assert_close(glow, low64.grad, EW, "dL/dlow")
        assert float(loss) == 0.0
    else:
        dd = d.double()     # (d is fp32 xhat - gt, the kernel's own difference; its p-th power is formed in double)
        assert_sum_bound(loss, dd.abs().pow(kind).sum(), dd.abs().pow(kind).sum(), 4, f"loss sum kind {kind}")
    # accumulate: added into existing gradients
    base = [(torch.randn(B, Cc, H, W, generator=g0).cuda(), torch.randn(B, Cc, H, W, generator=g0).cuda()) for _ in stages]
    acc = [(a.clone(), b.clone()) for a, b in base]
    ops.chain_inv_bwd(xhat.cuda(), gt.cuda(), stages, acc, gscale, loss_kind=kind, accumulate=True)
    for k, ((ds, dt), (b_s, b_t), (sr, tr)) in enumerate(zip(acc, base, leaves)):
        assert_close(ds, sr.grad + b_s.double().cpu(), EW, f"ds_raw accumulated stage {k}")
        assert_close(dt, tr.grad + b_t.double().cpu(), EW, f"dt_raw accumulated stage {k}")


def test_chain_inv_bwd_loss_sum_at_full_size():
    """The loss sum of a (1, 96, 512, 512) reconstruction: 49152 blocks, one float64 atomic each, under the reduction bound
    (k = 4: d = xhat - gt rounds once in fp32, its square / absolute value is exact in double)."""
    from cwfa_amd import ops
    shape = (1, 48, 512, 512)
    _, stages, _ = _chain_case(shape, 2, 5, "cuda")
    g0 = _gen(6)
    xhat, gt = _randn((1, 96, 512, 512), g0), _randn((1, 96, 512, 512), g0)
    grads = [(torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")) for _ in stages]
    for kind in (1, 2):
        loss = ops.chain_inv_bwd(xhat, gt, stages, grads, 1e-3, loss_kind=kind)
        d = (xhat - gt).double()
        p = d.abs().pow(kind).sum()
        assert_sum_bound(loss, p, p, 4, f"loss sum kind {kind}")


# ------------------------------------------------------------------------------------------------ composed: UNet with live Dropout2d
def test_unet_backward_with_live_dropout2d_vs_oracle():
    """UNet(5, 4, depth 3, wf 4, Dropout2d p = 0.3, bias) at 64x64, B = 2, train mode: per-sample A tables and masked BatchNorm
    statistics (g14 has drop_out = 0).  The masks come from fixed uniform draws on both sides; forward, input gradient and every
    parameter gradient against float64 autograd through the oracle.  A PReLU slope's gradient is one number, bounded by
    1e-5 * sum |g q-| over the reference's own terms (the upstream gradients are fp32, so the kernel's k 2**-24 bound does not
    apply to the composed sum)."""
    from oracle import cwfa_oracle as O
    from cwfa_amd import training, unet as U
    from conftest import rel_err
    torch.manual_seed(21)
    net = U.UNet(5, 4, depth=3, wf=4, drop_out=0.3, use_bias=True, skip_conn=True, up_mode="upconv", batch_norm=True)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.2, 0.2)
            if isinstance(mod, torch.nn.PReLU):
                mod.weight.fill_(0.2)
    sd0 = {k: v.detach().clone().double() for k, v in net.state_dict().items()}
    net = net.train().cuda()
    B = 2
    g0 = torch.Generator().manual_seed(22)
    x = torch.randn(B, 5, 64, 64, generator=g0)
    dy = torch.randn(B, 4, 64, 64, generator=g0)
    chans = [d.block[0].out_channels for d in list(net.down_path)[:-1]] + [u.conv_block.block[0].out_channels for u in net.up_path]
    draws = [torch.rand(B, c, generator=g0) for c in chans]
    assert all(bool((d < 0.3).any()) and bool((d >= 0.3).any()) for d in draws)
    pending = [d.clone() for d in draws]

    def fixed_mask(p, B_, C_, device):
        u = pending.pop(0)
        assert tuple(u.shape) == (B_, C_) and p == 0.3
        return ((u >= p).float() / (1.0 - p)).to(device)

    orig = U._drop_mask
    U._drop_mask = fixed_mask
    try:
        out, tape = training.unet_forward_train(net, x.cuda())
    finally:
        U._drop_mask = orig
    assert not pending
    gx = training.unet_backward(tape, dy.cuda())
    leaves = {k: v.requires_grad_(k.endswith("weight") or k.endswith("bias")) for k, v in sd0.items()}
    x64 = x.double().requires_grad_()
    # every PReLU of the float64 run records its input q and, on the way back, its upstream gradient g (for the slope bound)
    seen, real = [], F.prelu

    def recording_prelu(q, a):
        out = real(q, a)
        rec = {"a": a, "q": q.detach()}
        out.register_hook(lambda g: rec.__setitem__("g", g.detach()))
        seen.append(rec)
        return out

    F.prelu = recording_prelu
    try:
        ref = O.unet(leaves, x64, depth=3, train=True, drop_u=[d.double() for d in draws], drop_p=0.3)
    finally:
        F.prelu = real
    assert_close(out, ref.detach(), 1e-4, "train-mode forward with dropout")
    ref.backward(dy.double())
    assert_close(gx, x64.grad, 1e-4, "input gradient")
    got = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    want = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:6]
    bad = [(k, max(rel_err(got[k], want[k]))) for k in sorted(want) if want[k].numel() > 1 and not max(rel_err(got[k], want[k])) <= 1e-4]
    assert not bad, bad[:8]
    # PReLU slopes: d/dalpha = sum g * min(q, 0) over the layer, bounded with the reference's own terms
    slopes = [k for k in want if want[k].numel() == 1]
    assert len(slopes) == 11 and len(seen) == 11
    for k in slopes:
        rec = next(r for r in seen if r["a"] is leaves[k])
        terms = float((rec["g"] * torch.clamp(rec["q"], max=0)).abs().sum())
        assert abs(float(got[k]) - float(want[k])) <= 1e-5 * terms, (k, float(got[k]), float(want[k]), terms)
