"""The fused tail of the ConvNeXt block (cwfa_convnext_tail_f32 / ops.convnext_tail), the LayerNorm statistics from the few-channel
7x7's epilogue (cwfa_conv_opts.out_sample_stats) and the residual formed inside the tail (ops.CONVNEXT_RESIDUAL_FUSED).

The tail and the fused residual are held to torch.equal against the launches they replace (layernorm_apply -> scale_channels ->
the fp32 1x1 with GELU and residual; the fp32 1x1 launch that wrote u).  The epilogue statistics are float64 sums of the same fp32
values as ops.sample_stats of the launch's own output, in another order: with n <= 1e5 values the two differ by at most
n * 2^-53 ~ 1e-11 relative to sum|v| (sum v^2); the bound is 1e-10.  The module is held to the `within` bounds of
test_gpu_convnext_composed.py against a float64 evaluation."""
import ctypes as C

import pytest
import torch

from conftest import rel_err

NAN = float("nan")
NAN_BITS = torch.tensor(NAN).view(torch.int32).item()
EPS = 1e-5

# (B, C, H, W)
TAIL_CASES = [
    (2, 64, 19, 33),     # two m-tiles, a ragged last pixel tile, per-sample statistics
    (1, 6, 16, 16),      # the second block's width
    (2, 7, 9, 35),       # odd K, H*W not a multiple of 4
    (1, 10, 8, 32),      # exactly one tile per wave
    (3, 64, 8, 36),
]
# (B, c_in, c_out, H, W): the composed cases with Cin' <= 8
STAT_CASES = [(1, 6, 10, 16, 16), (2, 6, 64, 19, 33), (1, 3, 33, 9, 70), (1, 7, 64, 8, 32)]
GATES = [1.0 / 0.95, 0.0, 1.7]


def nan_around(shape, before, after):
    """a [B,C,H,W] view that is the channel slice [before, before + C) of a NaN-filled tensor; -> (view, whole allocation)"""
    B, Cc, H, W = shape
    flat = torch.full((B * (before + Cc + after) * H * W,), NAN, device="cuda")
    return flat.view(B, before + Cc + after, H, W)[:, before:before + Cc], flat


def untouched_outside(view, flat):
    probe = flat.clone()
    probe.as_strided(view.size(), view.stride(), view.storage_offset() - flat.storage_offset()).fill_(NAN)
    return bool((probe.view(torch.int32) == NAN_BITS).all())


def between_nans(t, before=2, after=3):
    view, _ = nan_around(tuple(t.shape), before, after)
    view.copy_(t)
    return view


_tail = {}


def tail_inputs(cfg):
    """the case's tensors on the device and the unfused sequence's results (per gate choice), computed once and left unchanged"""
    hit = _tail.get(cfg)
    if hit is None:
        from cwfa_amd import ops
        B, Cc, H, W = cfg
        g = torch.Generator().manual_seed(Cc + W)
        r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
        t = dict(v=between_nans(r(B, Cc, H, W) * 1.5 + 0.3), u=between_nans(r(B, Cc, H, W), 1, 2), lw=(1 + 0.1 * r(Cc, H, W)).cuda(),
                 lb=(0.1 * r(Cc, H, W)).cuda(), w1=(r(Cc, Cc, 1, 1) / Cc ** 0.5).cuda(), b1=(0.1 * r(Cc)).cuda(),
                 gate=torch.tensor(GATES[:B] if B > 1 else GATES[:1], dtype=torch.float32).cuda())
        t["st"] = ops.sample_stats(t["v"])
        vln = ops.layernorm_apply(t["v"], t["st"], t["lw"], t["lb"], EPS)
        pc = ops.pack_conv_weight(t["w1"])
        assert not pc.split
        res = ops.scale_channels(t["u"], t["gate"].reshape(B, 1).expand(B, Cc).contiguous())
        t["ref_gate"] = ops.conv2d(vln, pc, bias=t["b1"], act="gelu", residual=res)
        t["ref_none"] = ops.conv2d(vln, pc, bias=t["b1"], act="gelu", residual=t["u"])
        hit = _tail[cfg] = t
    return hit


@pytest.mark.gpu
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("cfg", TAIL_CASES, ids=str)
def test_tail_equals_the_unfused_sequence(cfg, gated):
    """bit for bit; y a slice of a NaN-filled buffer with nothing outside it written; NaN channels beside v and u do not leak; every
    sample alone equals its rows of the batch"""
    from cwfa_amd import ops
    B, Cc, H, W = cfg
    t = tail_inputs(cfg)
    gate = t["gate"] if gated else None
    ref = t["ref_gate" if gated else "ref_none"]
    out, flat = nan_around(cfg, 3, 2)
    y = ops.convnext_tail(t["v"], t["st"], t["lw"], t["lb"], EPS, t["w1"], t["b1"], u=t["u"], gate=gate, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    assert untouched_outside(out, flat), "a store outside the output slice"
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, ref)
    for s in range(B):
        ys = ops.convnext_tail(t["v"][s:s + 1], t["st"][2 * s:2 * s + 2], t["lw"], t["lb"], EPS, t["w1"], t["b1"], u=t["u"][s:s + 1],
                               gate=None if gate is None else gate[s:s + 1])
        assert torch.equal(ys, y[s:s + 1]), ("sample", s)


# ------------------------------------------------------------------------------------------------ statistics from the 7x7's epilogue
def composed_case(cfg):
    from cwfa_amd import ops
    B, cin, cout, H, W = cfg
    g = torch.Generator().manual_seed(cin + H)
    x = torch.randn(B, cin, H, W, generator=g)
    w0 = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    b0 = torch.randn(cout, generator=g) * 0.1
    w7 = torch.randn(cout, cout, 7, 7, generator=g) / (7 * cout ** 0.5)
    b7 = torch.randn(cout, generator=g) * 0.1
    x1 = between_nans(torch.cat([x, torch.ones(B, 1, H, W)], 1))
    pc = ops.pack_convnext_composed(w0.cuda(), b0.cuda(), w7.cuda())
    return x.cuda(), x1, w0.cuda(), b0.cuda(), pc, b7.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", STAT_CASES, ids=str)
def test_epilogue_statistics(cfg):
    """the buffer filled by the launch against ops.sample_stats of that launch's own output, per sample; asking for statistics leaves
    the output unchanged bit for bit"""
    from cwfa_amd import ops
    B = cfg[0]
    ops.set_precision("split_bf16")
    try:
        _, x1, _, _, pc, b7 = composed_case(cfg)
        assert ops.conv_writes_sample_stats(pc)
        plain = ops.conv2d(x1, pc, bias=b7)
        st = torch.zeros(2 * B, dtype=torch.float64, device="cuda")
        out, flat = nan_around(tuple(plain.shape), 3, 2)
        y = ops.conv2d(x1, pc, bias=b7, out=out, out_sample_stats=st)
        torch.cuda.synchronize()
        assert untouched_outside(out, flat)
        assert torch.equal(y, plain), "asking for statistics changed the output"
        ref = ops.sample_stats(y)
        yd = y.double()
        for b in range(B):
            sabs, ssq = yd[b].abs().sum().item(), (yd[b] * yd[b]).sum().item()
            d1, d2 = abs(st[2 * b].item() - ref[2 * b].item()), abs(st[2 * b + 1].item() - ref[2 * b + 1].item())
            print(f"epilogue stats {cfg} sample {b}: |d sum| / sum|v| = {d1 / sabs:.2e}, |d sumsq| / sum v^2 = {d2 / ssq:.2e}")
            assert d1 <= 1e-10 * sabs and d2 <= 1e-10 * ssq
    finally:
        ops.set_precision("fp32")


@pytest.mark.gpu
def test_other_forms_refuse_sample_statistics():
    """(1, 8, 48, 17, 40): Cin' = 9, the 25-step form -- conv_writes_sample_stats is false, ops.conv2d and the C entry point refuse the
    pointer; the fp32 entry point refuses it too"""
    from cwfa_amd import _lib, ops
    L = _lib.lib()
    ops.set_precision("split_bf16")
    try:
        _, x1, _, _, pc, b7 = composed_case((1, 8, 48, 17, 40))
        assert pc.cin == 9 and not ops.conv_writes_sample_stats(pc)
        st = torch.zeros(2, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            ops.conv2d(x1, pc, bias=b7, out_sample_stats=st)
        x1 = x1.contiguous()
        y = torch.empty(1, 48, 17, 40, device="cuda")
        o = _lib.ConvOpts()
        o.bias, o.out_sample_stats = b7.data_ptr(), st.data_ptr()
        ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        assert L.cwfa_conv7x7_split_f32(ptr(x1), ptr(pc.packed), ptr(y), 1, 9, 17, 40, 48, 9 * 17 * 40, 48 * 17 * 40, C.byref(o), None) != 0
        assert b"out_sample_stats" in L.cwfa_last_error()
    finally:
        ops.set_precision("fp32")
    w = torch.randn(48, 9, 1, 1).cuda()
    pc1 = ops.pack_conv_weight(w)
    assert not ops.conv_writes_sample_stats(pc1)
    assert L.cwfa_conv2d_f32(ptr(x1), ptr(pc1.packed), ptr(y), 1, 9, 17, 40, 48, 1, 9 * 17 * 40, 48 * 17 * 40, C.byref(o), None) != 0
    torch.cuda.synchronize()
    assert float(st.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ the residual formed in the tail
@pytest.mark.gpu
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("cfg", [(2, 6, 64, 19, 33), (1, 3, 33, 9, 70), (2, 6, 64, 8, 32)], ids=str)
def test_fused_residual_equals_the_1x1_launch(cfg, gated):
    """the tail with u formed from x is torch.equal to the tail reading the fp32 1x1 launch's u ((2, 6, 64, 8, 32): rows of whole
    16-byte words, the 1x1 kernel's vector-staged form, the one the 512 x 512 maps take); x sits between NaN channels"""
    from cwfa_amd import ops
    B, cin, Cc, H, W = cfg
    g = torch.Generator().manual_seed(cin + W)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    x = between_nans(r(B, cin, H, W))
    w0, b0 = (r(Cc, cin, 1, 1) / cin ** 0.5).cuda(), (0.1 * r(Cc)).cuda()
    v, lw, lb = (r(B, Cc, H, W) + 0.2).cuda(), (1 + 0.1 * r(Cc, H, W)).cuda(), (0.1 * r(Cc, H, W)).cuda()
    w1, b1 = (r(Cc, Cc, 1, 1) / Cc ** 0.5).cuda(), (0.1 * r(Cc)).cuda()
    gate = torch.tensor(GATES[:B], dtype=torch.float32).cuda() if gated else None
    st = ops.sample_stats(v)
    pc0 = ops.pack_conv_weight(w0)
    assert not pc0.split
    u = ops.conv2d(x, pc0, bias=b0)
    a = ops.convnext_tail(v, st, lw, lb, EPS, w1, b1, u=u, gate=gate)
    b = ops.convnext_tail(v, st, lw, lb, EPS, w1, b1, gate=gate, x=x, w0=w0, b0=b0)
    assert bool(torch.isfinite(b).all())
    assert torch.equal(a, b)


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
    m = N.ConvNeXt(6, cout, drop_prob=0.5, size=size)
    with torch.no_grad():
        m.m[1].weight.add_(0.1 * torch.randn(m.m[1].weight.shape))
        m.m[1].bias.add_(0.1 * torch.randn(m.m[1].bias.shape))
    x = torch.randn(3, 6, size, size)
    return m.cuda(), x


def within(y, ref, prec, what):
    """the bounds of test_gpu_convnext_composed.py: 1e-4 in both measures in split precision; bf16: max-rel 1e-2, l2-rel 5e-3"""
    m, l2 = rel_err(y, ref)
    print(f"{what} {prec}: max-rel {m:.2e}, l2-rel {l2:.2e}")
    if prec == "split_bf16":
        assert m <= 1e-4 and l2 <= 1e-4, (what, prec, m, l2)
    else:
        assert m <= 1e-2 and l2 <= 5e-3, (what, prec, m, l2)


OLD = ("cwfa_layernorm_apply_f32", "cwfa_scale_channels_f32", "cwfa_sample_stats_f32")


def count_launches(monkeypatch, L, names):
    seen = {n: 0 for n in names}
    for n in names:
        def wrap(*a, _n=n, _f=getattr(L, n)):
            seen[_n] += 1
            return _f(*a)
        monkeypatch.setattr(L, n, wrap)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["split_bf16", "bf16"])
@pytest.mark.parametrize("cout,size", [(64, 24), (10, 16)])
def test_convnext_module_tail_on_and_off(cout, size, prec, monkeypatch):
    """ConvNeXt(6, cout) in .train() (fixed CUDA seed) and in .eval(): with both paths handed ops.sample_stats' statistics the
    switches on and off give equal outputs; both stay within the bounds against float64 in eval mode; the fused path launches none
    of the three old kernels and no 1x1 for the residual"""
    from cwfa_amd import _lib, ops
    m, x = make_block(cout, size)
    ref = block64(m, x)
    xc = x.cuda()
    L = _lib.lib()
    seen = count_launches(monkeypatch, L, OLD + ("cwfa_conv2d_f32", "cwfa_convnext_tail_f32"))

    def run(tail, resid, train, same_stats):
        with monkeypatch.context() as mp:
            mp.setattr(ops, "CONVNEXT_TAIL_FUSED", tail)
            mp.setattr(ops, "CONVNEXT_RESIDUAL_FUSED", resid)
            if same_stats:
                mp.setattr(ops, "conv_writes_sample_stats", lambda pc: False)
            m.train(train)
            torch.cuda.manual_seed(11)
            for k in seen:
                seen[k] = 0
            with torch.no_grad():
                return m(xc)

    ops.set_precision(prec)
    try:
        for train in (True, False):
            off = run(False, True, train, True)
            assert seen["cwfa_convnext_tail_f32"] == 0 and seen["cwfa_layernorm_apply_f32"] == 1 and seen["cwfa_sample_stats_f32"] == 1
            assert seen["cwfa_scale_channels_f32"] == (1 if train else 0) and seen["cwfa_conv2d_f32"] == 2
            assert torch.equal(run(True, True, train, True), off), ("tail + residual fused", train)
            assert torch.equal(run(True, False, train, True), off), ("tail fused", train)
            if train:
                assert not torch.equal(off, run(False, True, False, True)), "the drop-path gate never showed"
            on = run(True, True, train, False)             # the path as shipped: statistics from the 7x7's epilogue
            assert seen == {**{k: 0 for k in seen}, "cwfa_convnext_tail_f32": 1}, seen
            run(True, False, train, False)
            assert seen == {**{k: 0 for k in seen}, "cwfa_convnext_tail_f32": 1, "cwfa_conv2d_f32": 1}, seen
            if not train:
                within(on, ref, prec, f"ConvNeXt(6, {cout}) fused tail vs float64")
                within(off, ref, prec, f"ConvNeXt(6, {cout}) unfused vs float64")
    finally:
        ops.set_precision("fp32")
        m.eval()


@pytest.mark.gpu
def test_training_path_keeps_the_old_kernels(monkeypatch):
    """the training forward and backward of the block (what AG.lrnn runs: training._convnext_forward_train / _convnext_backward)
    need the normalised map and u in memory: the three old entries are called, the fused tail is not"""
    from cwfa_amd import _lib, ops, training
    m, x = make_block(10, 16)
    m.train()
    L = _lib.lib()
    seen = count_launches(monkeypatch, L, OLD + ("cwfa_convnext_tail_f32",))
    ops.set_precision("split_bf16")
    try:
        torch.cuda.manual_seed(3)
        out, tape = training._convnext_forward_train(m, x.cuda())
        assert seen["cwfa_sample_stats_f32"] >= 1 and seen["cwfa_layernorm_apply_f32"] == 1 and seen["cwfa_scale_channels_f32"] == 1
        training._convnext_backward(tape, torch.ones_like(out), True)
        assert seen["cwfa_scale_channels_f32"] == 2 and seen["cwfa_convnext_tail_f32"] == 0
    finally:
        ops.set_precision("fp32")
        m.eval()
