"""The ConvNeXt block's 1x1 + 7x7 as ONE composed few-channel split 7x7 (ops.pack_convnext_composed, the few-channel forms of
cwfa_conv7x7_split_f32, the dispatch in networks.ConvNeXt.forward).

The reference of the kernel cases is conv2d(conv2d(x, w0, b0), w7, b7, padding=3) in float64 from the fp32 inputs; the bound is the
3e-6 (in assert_close's two measures) the split 7x7 family is held to (test_split_bf16_7x7_is_fp32_accurate), weights scaled as
there.

The floor of that bound -- compose in float64, round the bank ONCE to fp32, convolve in float64: what the re-association costs
before any kernel runs -- measured on the CPU for the seeds below (test_rounding_floor_of_the_composed_bank asserts it stays under
a third of the bound), (max-rel, l2-rel) per case:
    (1, 6, 10, 16, 16)   2.20e-08, 2.44e-08
    (2, 6, 64, 19, 33)   2.87e-08, 2.53e-08
    (1, 3, 33, 9, 70)    2.43e-08, 2.42e-08
    (1, 7, 64, 8, 32)    2.90e-08, 2.48e-08
    (1, 8, 48, 17, 40)   2.86e-08, 2.52e-08
    (2, 15, 64, 24, 31)  2.64e-08, 2.52e-08
(the Cin' = 17 case is not composed).  The floor is two orders of magnitude under the bound: the bound is the kernel's."""
import pytest
import torch

from conftest import assert_close, rel_err

NAN = float("nan")
NAN_BITS = torch.tensor(NAN).view(torch.int32).item()
BOUND = 3e-6

# (B, c_in, c_out, H, W)
CASES = [
    (1, 6, 10, 16, 16),      # the golden's shape
    (2, 6, 64, 19, 33),      # ragged rows and columns, batch > 1
    (1, 3, 33, 9, 70),       # one row tile, three column tiles, odd cout
    (1, 7, 64, 8, 32),       # Cin' = 8, exactly one tile
    (1, 8, 48, 17, 40),      # Cin' = 9, first trimmed case
    (2, 15, 64, 24, 31),     # Cin' = 16
    (1, 16, 64, 16, 32),     # Cin' = 17: NOT composed, the two-stage path
]
_cache = {}


def inputs(cfg):
    """the case's fp32 tensors and its float64 reference, computed once and shared"""
    hit = _cache.get(cfg)
    if hit is None:
        B, cin, cout, H, W = cfg
        g = torch.Generator().manual_seed(cin + H)
        x = torch.randn(B, cin, H, W, generator=g)
        w0 = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
        b0 = torch.randn(cout, generator=g) * 0.1
        w7 = torch.randn(cout, cout, 7, 7, generator=g) / (7 * cout ** 0.5)
        b7 = torch.randn(cout, generator=g) * 0.1
        F = torch.nn.functional
        ref = F.conv2d(F.conv2d(x.double(), w0.double(), b0.double()), w7.double(), b7.double(), padding=3)
        hit = _cache[cfg] = dict(x=x, w0=w0, b0=b0, w7=w7, b7=b7, ref=ref)
    return hit


def composed_fp32_bank(t):
    """[W0 | b0] composed with W7 in float64, rounded once to fp32: [cout, cin + 1, 7, 7]"""
    cout, cin = t["w0"].shape[:2]
    w0p = torch.cat([t["w0"].reshape(cout, cin).double(), t["b0"].double().reshape(cout, 1)], 1)
    return torch.einsum("omt,mi->oit", t["w7"].double().reshape(cout, cout, 49), w0p).reshape(cout, cin + 1, 7, 7).float()


@pytest.mark.parametrize("cfg", CASES[:-1], ids=str)
def test_rounding_floor_of_the_composed_bank(cfg):
    """compose in float64, round the bank to fp32, convolve in float64: the part of the bound that owes nothing to the kernel"""
    t = inputs(cfg)
    x1 = torch.cat([t["x"], torch.ones_like(t["x"][:, :1])], 1).double()
    got = torch.nn.functional.conv2d(x1, composed_fp32_bank(t).double(), t["b7"].double(), padding=3)
    m, l2 = rel_err(got, t["ref"])
    print(f"floor {cfg}: max-rel {m:.2e}, l2-rel {l2:.2e}")
    assert m <= BOUND / 3 and l2 <= BOUND / 3


# ------------------------------------------------------------------------------------------------ device layouts
def nan_around(shape, before, after):
    """a [B,C,H,W] view that is the channel slice [before, before + C) of a NaN-filled tensor; -> (view, whole allocation)"""
    B, Cc, H, W = shape
    flat = torch.full((B * (before + Cc + after) * H * W,), NAN, device="cuda")
    return flat.view(B, before + Cc + after, H, W)[:, before:before + Cc], flat


def untouched_outside(view, flat):
    probe = flat.clone()
    probe.as_strided(view.size(), view.stride(), view.storage_offset() - flat.storage_offset()).fill_(NAN)
    return bool((probe.view(torch.int32) == NAN_BITS).all())


def conv_pair(ops, t, x=None, out=None):
    """v = conv7x7(conv1x1(x) + b0) + b7 the way networks.ConvNeXt.forward dispatches it; ``x``: the input, for the composed form WITH
    its ones channel (a view between NaN channels)"""
    cout, cin = t["w0"].shape[:2]
    b7 = t["b7"].cuda()
    if ops.convnext_composed(cin, cout):
        pc = ops.pack_convnext_composed(t["w0"].cuda(), t["b0"].cuda(), t["w7"].cuda())
        assert pc.split and pc.ks == 7 and pc.cin == cin + 1
        return ops.conv2d(x, pc, bias=b7, out=out)
    u = ops.conv2d(x, ops.pack_conv_weight(t["w0"].cuda()), bias=t["b0"].cuda())
    return ops.conv2d(u, ops.pack_conv_weight(t["w7"].cuda()), bias=b7, out=out)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["split_bf16"])
@pytest.mark.parametrize("cfg", CASES, ids=str)
def test_composed_7x7_vs_float64(cfg, fmt, monkeypatch):
    """the float64 bound; the output a slice of a NaN-filled buffer with nothing outside it written; NaN channels next to the input
    in memory do not leak (the ones channel is the LAST channel the kernel may read); every sample alone bit-equal to the batch"""
    from cwfa_amd import _lib, ops
    B, cin, cout, H, W = cfg
    t = inputs(cfg)
    L = _lib.lib()
    seen = []
    k7 = L.cwfa_conv7x7_split_f32
    monkeypatch.setattr(L, "cwfa_conv7x7_split_f32", lambda *a: (seen.append(a[4]), k7(*a))[1])
    ops.set_precision(fmt)
    try:
        composed = ops.convnext_composed(cin, cout)
        assert composed == (cin + 1 <= 16)
        if composed:
            x1 = torch.cat([t["x"], torch.ones(B, 1, H, W)], 1)
            x, _ = nan_around(tuple(x1.shape), 2, 3)
            x.copy_(x1)
        else:
            with pytest.raises(ValueError):
                ops.pack_convnext_composed(t["w0"].cuda(), t["b0"].cuda(), t["w7"].cuda())
            x, _ = nan_around(tuple(t["x"].shape), 2, 3)
            x.copy_(t["x"])
        out, flat = nan_around((B, cout, H, W), 3, 2)
        y = conv_pair(ops, t, x, out)
        torch.cuda.synchronize()
        assert y.data_ptr() == out.data_ptr()
        assert seen == [cin + 1 if composed else cout], "the 7x7 launch did not read the expected number of channels"
        assert untouched_outside(out, flat), "a store outside the output slice"
        m, l2 = rel_err(y, t["ref"])
        print(f"composed 7x7 {cfg} {fmt}: max-rel {m:.2e}, l2-rel {l2:.2e}, bound {BOUND:g}")
        assert_close(y, t["ref"], BOUND, f"composed 7x7 {cfg} vs float64")
        for s in range(B):
            assert torch.equal(conv_pair(ops, t, x[s:s + 1]), y[s:s + 1]), ("sample", s)
    finally:
        ops.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ the module
def block64(m, x):
    """networks.ConvNeXt in eval mode (drop_path = identity), float64"""
    F = torch.nn.functional
    d = lambda p: p.detach().double().cpu()   # noqa: E731
    u = F.conv2d(x.double(), d(m.input.weight), d(m.input.bias))
    v = F.conv2d(u, d(m.m[0].weight), d(m.m[0].bias), padding=3)
    v = F.layer_norm(v, v.shape[1:], d(m.m[1].weight), d(m.m[1].bias), m.m[1].eps)
    return F.gelu(F.conv2d(v, d(m.m[2].weight), d(m.m[2].bias))) + u


def make_block(cout, size, seed=5):
    from cwfa_amd import networks as N
    torch.manual_seed(seed)
    m = N.ConvNeXt(6, cout, drop_prob=0.05, size=size)
    with torch.no_grad():
        m.m[1].weight.add_(0.1 * torch.randn(m.m[1].weight.shape))
        m.m[1].bias.add_(0.1 * torch.randn(m.m[1].bias.shape))
    x = torch.randn(2, 6, size, size)
    return m.eval().cuda(), x


def within(y, ref, prec, what):
    """the bounds test_gpu_parity.py holds the LRNN's outputs to: 1e-4 in both measures in split precision; bf16: max-rel 1e-2,
    l2-rel 5e-3"""
    m, l2 = rel_err(y, ref)
    print(f"{what} {prec}: max-rel {m:.2e}, l2-rel {l2:.2e}")
    if prec == "split_bf16":
        assert m <= 1e-4 and l2 <= 1e-4, (what, prec, m, l2)
    else:
        assert m <= 1e-2 and l2 <= 5e-3, (what, prec, m, l2)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["split_bf16", "bf16"])
@pytest.mark.parametrize("cout,size", [(64, 24), (10, 16)])
def test_convnext_module_composed_on_and_off(cout, size, prec, monkeypatch):
    """ConvNeXt(6, cout).eval(): CONVNEXT_COMPOSED on and off against a float64 evaluation of the module and against each other;
    the composed form launches the 7x7 over 7 channels, the two-stage form over cout"""
    from cwfa_amd import _lib, ops
    m, x = make_block(cout, size)
    ref = block64(m, x)
    L = _lib.lib()
    seen = []
    k7 = L.cwfa_conv7x7_split_f32
    monkeypatch.setattr(L, "cwfa_conv7x7_split_f32", lambda *a: (seen.append(a[4]), k7(*a))[1])
    ops.set_precision(prec)
    try:
        with torch.no_grad():
            monkeypatch.setattr(ops, "CONVNEXT_COMPOSED", True)
            on = m(x.cuda())
            assert seen == [7]
            monkeypatch.setattr(ops, "CONVNEXT_COMPOSED", False)
            off = m(x.cuda())
            assert seen == ([7, 64] if cout == 64 else [7])       # (10 -> 10: not a split 7x7 bank, the fp32 MFMA kernel)
    finally:
        ops.set_precision("fp32")
    within(on, ref, prec, f"ConvNeXt(6, {cout}) composed vs float64")
    within(off, ref, prec, f"ConvNeXt(6, {cout}) two-stage vs float64")
    within(on, off, prec, f"ConvNeXt(6, {cout}) composed vs two-stage")


@pytest.mark.gpu
def test_composed_bank_follows_its_sources(monkeypatch):
    """an in-place edit of m[0].weight, input.bias or input.weight (optimiser-style add_) and ops.invalidate_packs() each rebuild the
    composed bank: the result moves with the parameters and matches the two-stage path on the same parameters"""
    from cwfa_amd import ops
    m, x = make_block(10, 16, seed=6)
    x = x.cuda()
    packs = []
    pack = ops.pack_convnext_composed
    monkeypatch.setattr(ops, "pack_convnext_composed", lambda *a: (packs.append(1), pack(*a))[1])

    def two_stage():
        monkeypatch.setattr(ops, "CONVNEXT_COMPOSED", False)
        try:
            return m(x)
        finally:
            monkeypatch.setattr(ops, "CONVNEXT_COMPOSED", True)

    ops.set_precision("split_bf16")
    try:
        with torch.no_grad():
            y = m(x)
            assert len(packs) == 1
            assert torch.equal(m(x), y) and len(packs) == 1, "an unchanged block re-packed its bank"
            g = torch.Generator(device="cuda").manual_seed(1)
            for n, p in enumerate((m.m[0].weight, m.input.bias, m.input.weight), start=2):
                p.add_(0.05 * torch.randn(p.shape, generator=g, device="cuda"))
                y1 = m(x)
                assert len(packs) == n, "the bank was not rebuilt"
                assert not torch.equal(y1, y)
                within(y1, two_stage(), "split_bf16", "after an in-place edit")
                y = y1
            m.m[0].weight.data.mul_(0.5)              # no version bump: the caches cannot see it ...
            assert torch.equal(m(x), y) and len(packs) == 4
            ops.invalidate_packs()                    # ... until they are told
            y1 = m(x)
            assert len(packs) == 5 and not torch.equal(y1, y)
            within(y1, two_stage(), "split_bf16", "after invalidate_packs")
    finally:
        ops.set_precision("fp32")
