"""GPU (MI355X): the fp16 precision mode (ops.set_precision("fp16"), cwfa_amd.install(precision="fp16")) -- the arithmetic of the
reference's default --use_half_precision 1 (CUDA autocast: fp16 operands, fp32 accumulation).

Kernel units are held to a float64 convolution of the fp16-ROUNDED operands (torch's .half(): round to nearest even, +-inf beyond
+-65504) at max-rel <= 2e-5, which leaves only the fp32 accumulation error; each case also shows that the bf16-rounded reference is
at least 10x further away (fp16 really ran).  The load-side prologue is applied in fp32, in the kernel's order, before rounding."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from split_ref import F16_TOL, _pro32, b16, check16, h, maxrel, pack_split3x3


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _restore_precision():
    from cwfa_amd import ops
    yield
    ops.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ kernel units
@pytest.mark.parametrize("cfg", [(1, 70, 16, 32, 200), (2, 33, 9, 37, 130), (1, 256, 24, 64, 512)])
def test_fp16_1x1_gemm(cfg):
    """cwfa_split_input_f32 (one fp16 plane, with the load-side affine + added tensor) and the 1x1 GEMM on the f16 32x32x16 form"""
    from cwfa_amd import ops
    B, Cin, H, W, Cout = cfg
    g = torch.Generator().manual_seed(Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    b = torch.randn(Cout, generator=g)
    res = torch.randn(B, Cout, H, W, generator=g)
    sc, sh = torch.rand(B, Cin, generator=g) + 0.5, torch.randn(B, Cin, generator=g)
    add = torch.randn(B, Cin, H, W, generator=g)
    alpha = torch.tensor([0.2])
    ops.set_precision("fp16")
    pc = ops.pack_conv_weight(w.cuda())
    assert pc.split
    y = ops.conv2d(x.cuda(), pc, bias=b.cuda())
    y2 = ops.conv2d(x.cuda(), pc, bias=b.cuda(), act="elu", residual=res.cuda(), act2="elu")
    y3 = ops.conv2d(x.cuda(), pc, bias=b.cuda(), act="prelu", prelu_alpha=alpha.cuda(), in_scale=sc.cuda(), in_shift=sh.cuda(), in_add=add.cuda())
    xp = x * sc.view(B, -1, 1, 1) + sh.view(B, -1, 1, 1) + add
    for rnd, name in ((h, "fp16"), (b16, "bf16")):
        ref = F.conv2d(rnd(x), rnd(w), b.double())
        if name == "fp16":
            rh = (ref, F.elu(F.elu(ref) + res.double()), F.prelu(F.conv2d(rnd(xp), rnd(w), b.double()), alpha.double()))
        else:
            rb = (ref, F.elu(F.elu(ref) + res.double()), F.prelu(F.conv2d(rnd(xp), rnd(w), b.double()), alpha.double()))
    for got, a, c, what in zip((y, y2, y3), rh, rb, ("plain", "elu+res+elu", "prologue+prelu")):
        check16(got, a, c, f"1x1 {cfg} {what}")


def test_fp16_conv_transpose():
    from cwfa_amd import ops
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 40, 9, 16, generator=g)
    w = torch.randn(40, 48, 2, 2, generator=g) * 0.2
    b = torch.randn(48, generator=g)
    ops.set_precision("fp16")
    pc = ops.pack_conv_weight(w.cuda(), transposed=True)
    assert pc.split
    y = ops.conv2d(x.cuda(), pc, bias=b.cuda())
    ct = lambda r: F.conv_transpose2d(r(x), r(w), b.double(), stride=2)     # noqa: E731
    check16(y, ct(h), ct(b16), "transposed")


@pytest.mark.parametrize("cfg", [(1, 70, 7, 63, 200), (1, 256, 8, 64, 256), (2, 20, 12, 37, 320), (1, 6, 19, 40, 256),
                                 (1, 48, 9, 33, 130), (2, 33, 17, 50, 520), (1, 64, 16, 32, 96), (1, 64, 5, 20, 12),
                                 (1, 64, 33, 50, 24), (2, 29, 20, 40, 6), (1, 24, 16, 32, 32), (1, 64, 40, 64, 17), (1, 29, 9, 12, 16),
                                 (1, 64, 16, 64, 64), (1, 64, 20, 36, 48)])
def test_fp16_3x3(cfg):
    """the split 3x3 kernel with fp16 operands: 256 / 128 / 64-channel tilings (8- and 16-row tiles), the narrow tilings, ragged
    edges (W % 4 == 0 and != 0), the skip-add / affine prologue, the specialised and run-time epilogues"""
    from cwfa_amd import ops
    B, Cin, H, W, Cout = cfg
    g = torch.Generator().manual_seed(Cin * 3 + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    res = torch.randn(B, Cout, H, W, generator=g)
    alpha = torch.tensor([0.2])
    sc, sh = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g)
    add = torch.randn(B, Cin, H, W, generator=g)
    narrow = Cout <= 48 or 64 < Cout <= 96
    ops.set_precision("fp16")
    keep_min = ops.SPLIT_3X3_MIN_COUT
    ops.SPLIT_3X3_MIN_COUT = 1
    try:
        pc = pack_split3x3(ops, w.cuda())
        assert pc.split
        got = {"plain": ops.conv2d(x.cuda(), pc, bias=b.cuda()),
               "prelu": ops.conv2d(x.cuda(), pc, bias=b.cuda(), act="prelu", prelu_alpha=alpha.cuda()),
               "generic": ops.conv2d(x.cuda(), pc, bias=b.cuda(), act="gelu", residual=res.cuda(), act2="relu")}
        if not narrow:
            got["pro_prelu"] = ops.conv2d(x.cuda(), pc, bias=b.cuda(), act="prelu", prelu_alpha=alpha.cuda(), in_scale=sc.cuda(),
                                          in_shift=sh.cuda(), in_add=add.cuda())
            got["aff_prelu"] = ops.conv2d(x.cuda(), pc, bias=b.cuda(), act="prelu", prelu_alpha=alpha.cuda(), in_scale=sc.cuda(),
                                          in_shift=sh.cuda())
    finally:
        ops.SPLIT_3X3_MIN_COUT = keep_min

    def want(rnd):
        ref = F.conv2d(rnd(x), rnd(w), b.double(), padding=1)
        out = {"plain": ref, "prelu": F.prelu(ref, alpha.double()), "generic": F.relu(F.gelu(ref) + res.double())}
        out["pro_prelu"] = F.prelu(F.conv2d(rnd(_pro32(x, sc, sh, add)), rnd(w), b.double(), padding=1), alpha.double())
        out["aff_prelu"] = F.prelu(F.conv2d(rnd(_pro32(x, sc, sh)), rnd(w), b.double(), padding=1), alpha.double())
        return out
    wh, wb = want(h), want(b16)
    for k in got:
        check16(got[k], wh[k], wb[k], f"3x3 {cfg} {k}")


def test_fp16_subnormal_operands():
    """Operands in the fp16 subnormal range (|v| < 2^-14): the reference keeps them (torch's .half() does; so does autocast).
    The kernel is compared with that reference and with the flushed one (subnormal operands -> 0); DESIGN.md section 11."""
    from cwfa_amd import ops
    g = torch.Generator().manual_seed(77)
    B, Cin, H, W, Cout = 1, 64, 16, 32, 128
    x = torch.randn(B, Cin, H, W, generator=g) * 2.0 ** -17        # |x| ~ 1e-5: fp16 subnormals (min normal 6.1e-5)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    ops.set_precision("fp16")
    y = ops.conv2d(x.cuda(), ops.pack_conv_weight(w.cuda()))
    xh = h(x)
    assert float((xh.abs() < 2.0 ** -14).double().mean()) > 0.9
    keep = F.conv2d(xh, h(w), padding=1)
    ftz = F.conv2d(torch.where(xh.abs() < 2.0 ** -14, torch.zeros_like(xh), xh), h(w), padding=1)
    e_keep, e_ftz = maxrel(y, keep), maxrel(y, ftz)
    print(f"subnormal operands: max-rel vs kept {e_keep:.3e}, vs flushed {e_ftz:.3e}")
    assert e_keep <= F16_TOL and e_ftz > 100 * e_keep, (e_keep, e_ftz)
    # overflow: beyond +-65504 an operand becomes +-inf, as .half() makes it
    x2 = torch.zeros(1, 64, 4, 8)
    x2[0, 3, 1, 2] = 70000.0
    w2 = torch.zeros(128, 64, 3, 3)
    w2[5, 3, 1, 1] = 1.0
    y2 = ops.conv2d(x2.cuda(), ops.pack_conv_weight(w2.cuda())).cpu()
    assert torch.isinf(y2[0, 5, 1, 2]) and float(y2[0, 5, 1, 2]) > 0


@pytest.mark.parametrize("cfg", [(1, 64, 64, 40, 70), (2, 40, 33, 19, 33), (1, 32, 64, 8, 32)])
def test_fp16_7x7(cfg):
    from cwfa_amd import ops
    B, cin, cout, H, W = cfg
    g = torch.Generator().manual_seed(cin + H)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 7, 7, generator=g) / (7 * cin ** 0.5)
    bias = torch.randn(cout, generator=g) * 0.1
    ops.set_precision("fp16")
    pc = ops.pack_conv_weight(w.cuda())
    assert pc.split and pc.ks == 7
    y = ops.conv2d(x.cuda(), pc, bias=bias.cuda())
    ref = lambda r: F.conv2d(r(x), r(w), bias.double(), padding=3)     # noqa: E731
    check16(y, ref(h), ref(b16), f"7x7 {cfg}")


@pytest.mark.parametrize("cfg", [(1, 24, 64, 40, 72, "ATAN", 1.0, False), (2, 48, 64, 33, 50, "TANH", 0.1, True)])
def test_fp16_coupling_epilogue(cfg):
    from cwfa_amd import ops
    B, n, cin, H, W, kind, pre, rev = cfg
    g = torch.Generator().manual_seed(n + H)
    w = torch.randn(2 * n, cin, 3, 3, generator=g) * (1.5 / (3 * cin ** 0.5))
    bias = torch.randn(2 * n, generator=g) * 0.1
    u = torch.randn(B, cin, H, W, generator=g)
    x = torch.randn(B, n, H, W, generator=g)
    clamp = 1.7

    def ref(rnd):
        a = F.conv2d(rnd(u), rnd(w), bias.double(), padding=1) * pre
        s = {"ATAN": lambda v: clamp * 0.636 * torch.atan(v), "TANH": lambda v: clamp * torch.tanh(v)}[kind](a[:, :n])
        t = a[:, n:]
        return (x.double() - t) * torch.exp(-s) if rev else torch.exp(s) * x.double() + t
    ops.set_precision("fp16")
    bank = ops.pack_couple_weight(w.cuda(), bias.cuda())
    out = torch.empty(B, n, H, W, device="cuda")
    ops.conv3x3_couple(u.cuda(), bank, x.cuda(), out, kind, clamp, pre, rev)
    # (the soft clamp's fast atan / tanh and the hardware exp add ~3e-7 absolute: within the bound)
    check16(out, ref(h), ref(b16), f"coupling epilogue {cfg}")


def _layer_ref(rnd, x, w3, b3, w1, b1):
    hid = F.elu(F.conv2d(rnd(x), rnd(w3), b3.double(), padding=1))
    return F.elu(F.conv2d(rnd(hid.float()), rnd(w1), b1.double()) + x.double()), hid


@pytest.mark.parametrize("shape", [(1, 32, 32), (2, 17, 45), (1, 70, 96), (2, 130, 200)])
def test_fp16_fused_layer(shape):
    """the fused sub-network layer: NCHW, the channel-blocked layouts (bit-identical to NCHW) and the tape form (hidden map)"""
    from cwfa_amd import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(H * W + 1)
    x = torch.randn(B, 64, H, W, generator=g)
    w3, b3 = torch.randn(64, 64, 3, 3, generator=g) / 24, torch.randn(64, generator=g) * 0.1
    w1, b1 = torch.randn(64, 64, 1, 1, generator=g) / 8, torch.randn(64, generator=g) * 0.1
    ops.set_precision("fp16")
    pc = ops.pack_split_layer_weight(w3.cuda(), w1.cuda())
    y = ops.subnet_layer(x.cuda(), pc, b3.cuda(), None, b1.cuda())
    yt, hid = ops.subnet_layer(x.cuda(), pc, b3.cuda(), None, b1.cuda(), want_hidden=True)
    assert torch.equal(yt, y)
    _, hh = _layer_ref(h, x, w3, b3, w1, b1)
    _, hb = _layer_ref(b16, x, w3, b3, w1, b1)
    check16(hid, hh, hb, f"hidden map of the tape form {shape}")
    # the 1x1 phase against the kernel's own fp32 hidden map, rounded: a float64 hidden map rounds to a different fp16 neighbour
    # wherever the fp32 accumulation error straddles a rounding boundary (one fp16 ulp, 2^-11 relative, on that element)
    hk = hid.cpu()
    y1 = lambda r: F.elu(F.conv2d(r(hk), r(w1), b1.double()) + x.double())     # noqa: E731
    check16(y, y1(h), y1(b16), f"fused layer {shape}")
    xb = _to_blocked(x.cuda())
    for layout in (1, 2, 3):
        yo = ops.subnet_layer(xb if layout & 1 else x.cuda(), pc, b3.cuda(), None, b1.cuda(), layout=layout)
        assert torch.equal(_from_blocked(yo) if layout & 2 else yo, y), layout


@pytest.mark.parametrize("cin", [7, 20])
@pytest.mark.parametrize("shape", [(1, 32, 32), (2, 17, 45)])
def test_fp16_composed_first_layer(cin, shape):
    """the first layer of a sub-network with the 1x1 in front composed into its 3x3 (float64, rounded to fp32 once): the composed
    weights are what is rounded to fp16 (the reference rounds W0 and W3 separately -- DESIGN.md section 11).  Forms: residual
    given, residual formed in the launch (fused first map), and the short form (cin + 1 <= 16)."""
    from cwfa_amd import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(cin * 100 + H)
    u = torch.randn(B, cin, H, W, generator=g)
    w0, b0 = torch.randn(64, cin, 1, 1, generator=g) / cin ** 0.5, torch.randn(64, generator=g) * 0.1
    w3, b3 = torch.randn(64, 64, 3, 3, generator=g) / 24, torch.randn(64, generator=g) * 0.1
    w1, b1 = torch.randn(64, 64, 1, 1, generator=g) / 8, torch.randn(64, generator=g) * 0.1
    u1 = torch.cat([u, torch.ones(B, 1, H, W)], 1)
    w0p = torch.cat([w0.reshape(64, cin).double(), b0.double().reshape(64, 1)], 1)
    w3c = torch.einsum("omt,mi->oit", w3.double().reshape(64, 64, 9), w0p).reshape(64, cin + 1, 3, 3).float()
    x = F.conv2d(u, w0, b0)                                          # the residual, when it is given (fp32)
    ops.set_precision("fp16")
    forms = {}
    for short in ((False, True) if cin + 1 <= 16 else (False,)):
        pc = ops.pack_first_layer_weight(w0.cuda(), b0.cuda(), w3.cuda(), w1.cuda(), short=short)
        if not short:
            forms["given x"] = (ops.subnet_layer_first(u1.cuda(), x.cuda(), pc, b3.cuda(), b1.cuda()), False)
        forms["fused x" + (" short" if short else "")] = (ops.subnet_layer_first(u1.cuda(), None, pc, b3.cuda(), b1.cuda()), True)

    def ref(rnd, fused):
        hid = F.elu(F.conv2d(rnd(u1), rnd(w3c), b3.double(), padding=1))
        xr = F.conv2d(rnd(u1), rnd(w0p.float()).reshape(64, cin + 1, 1, 1)) if fused else x.double()
        return F.elu(F.conv2d(rnd(hid.float()), rnd(w1), b1.double()) + xr)
    # (bound: the hidden map is rounded to fp16 inside the launch, from fp32 accumulators -- where the float64 reference's hidden
    # value lies on the other side of a rounding boundary the element differs by one fp16 ulp; see test_fp16_fused_layer, whose
    # tape form exposes the hidden map and pins each phase at 2e-5)
    for k, (y, fused) in forms.items():
        check16(y, ref(h, fused), ref(b16, fused), f"composed first layer, {k}, cin {cin}, {shape}", tol=2.5e-4)


def _to_blocked(t):
    B, Cc, H, W = t.shape
    return t.view(B, Cc // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().view(B, Cc, H, W)


def _from_blocked(t):
    B, Cc, H, W = t.shape
    return t.view(B, Cc // 8, H, W, 8).permute(0, 1, 4, 2, 3).contiguous().view(B, Cc, H, W)


@pytest.mark.parametrize("cfg", [(1, 6, 9, 11, 4, 0.25), (2, 8, 16, 40, 32, 0.25), (1, 12, 8, 32, 32, -0.5), (2, 3, 29, 31, 17, 1.0)])
def test_fp16_conv3d(cfg):
    from cwfa_amd import ops
    B, D, H, W, K, alpha = cfg
    g = torch.Generator().manual_seed(K + D)
    x = torch.randn(B, D, H, W, generator=g)
    w1, b1 = torch.randn(K, 1, 3, 3, 3, generator=g) * 0.3, torch.randn(K, generator=g) * 0.1
    w2, b2 = torch.randn(1, K, 3, 3, 3, generator=g) * 0.1, torch.randn(1, generator=g)
    a = torch.tensor([alpha])
    ops.set_precision("fp16")
    y = ops.conv3d_1k1(*[t.cuda() for t in (x, w1, b1, a, w2, b2)])

    def ref(rnd):
        v = rnd(x).permute(0, 2, 3, 1).unsqueeze(1)
        hid = F.prelu(F.conv3d(v, rnd(w1), b1.double(), padding=1), a.double())
        v = F.conv3d(rnd(hid.float()), rnd(w2), b2.double(), padding=1)
        return v[:, 0].permute(0, 3, 1, 2)
    check16(y, ref(h), ref(b16), f"conv3d {cfg}", tol=2.5e-4)      # (hidden map rounded in the launch: test_fp16_composed_first_layer)


# ------------------------------------------------------------------------------------------------ options
def test_option_pairs_and_mode_cycle():
    from cwfa_amd import _lib, ops
    L = _lib.lib()
    ops.set_precision("split_bf16")
    assert L.cwfa_set_option(b"split_operand", 1) == -1                # CWFA_E_INVAL
    ops.set_precision("fp16")
    assert L.cwfa_set_option(b"split_products", 6) == -1
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 64, 24, 40, generator=g).cuda()
    w = (torch.randn(128, 64, 3, 3, generator=g) / 24).cuda()

    def run(mode):
        ops.set_precision(mode)
        return ops.conv2d(x, ops.pack_conv_weight(w))
    fresh = run("split_bf16")
    outs = [run(m) for m in ("fp32", "fp16", "bf16", "split_bf16", "fp32")]
    assert torch.equal(outs[3], fresh)
    assert not torch.equal(outs[1], outs[2]) and not torch.equal(outs[1], fresh)


# ------------------------------------------------------------------------------------------------ the modes end to end
def test_full_config3_inverse_fp16_vs_oracle():
    """BASELINE.json configs[2] at full size (512x512x96, LRNN + 4 flow steps, stochastic layers off) in fp16 against the fp32 CPU
    oracle, and the bf16 mode on the same inputs: fp16's L2 error is at most half of bf16's.  Also the LRNN Encoder under autocast."""
    from cwfa_amd import CWFA, ops
    from oracle import cwfa_oracle as O
    torch.manual_seed(0)
    np.random.seed(0)
    conv_inn, cond_nets = CWFA.build_networks(96, 512, 5, with_lrnn=True, device="cuda")
    enc = cond_nets[-1]
    enc.net.deconv[1].drop_out = 0
    for cn in enc.net.conv3d:
        cn.drop_prob = 0.0
    g = torch.Generator().manual_seed(1)
    cond_input = torch.randn(1, 29, 512, 512, generator=g)
    mean_cache = [0.1 * torch.randn(1, 96 // 2 ** (n + 1), 512, 512, generator=g) for n in range(4)]
    cpu = lambda sd: {k: v.detach().cpu() for k, v in sd.items()}   # noqa: E731
    steps = []
    for n, gi in enumerate(conv_inn):
        axes = {i: (m.axis if hasattr(m, "axis") else 1) for i, m in enumerate(gi.module_list) if hasattr(m, "perm")}
        steps.append({"inn": cpu(gi.state_dict()), "omega": cpu(cond_nets[n].state_dict()), "axes": axes})
    outs = {}
    for prec in ("fp16", "bf16"):
        ops.set_precision(prec)
        with torch.no_grad():
            outs[prec] = CWFA.inverse_pass(conv_inn, cond_nets, cond_input.cuda(), [m.cuda() for m in mean_cache])
        torch.cuda.synchronize()
    ops.set_precision("fp16")
    with torch.no_grad():
        e0 = enc(cond_input.cuda(), mean_cache[-1].cuda())[-1]
        with torch.autocast("cuda", dtype=torch.float16):
            e1 = enc(cond_input.cuda(), mean_cache[-1].cuda())[-1]
    assert e1.dtype == torch.float32 and torch.equal(e0, e1), "LRNN Encoder under autocast"
    with torch.no_grad():
        ref = O.inverse_pass(steps, None, cond_input, mean_cache, lrnn_sd=cpu(enc.state_dict()), lrnn_train=True)[-1]
    err = {}
    for prec, out in outs.items():
        mr = maxrel(out, ref)
        l2 = float((out.double().cpu() - ref.double()).norm() / ref.double().norm())
        err[prec] = (mr, l2)
        print(f"full-size config-3 inverse, {prec}: max-rel {mr:.3e}, L2-rel {l2:.3e}")
    assert err["fp16"][0] <= 2.5e-3 and err["fp16"][1] <= 1e-3, err
    assert err["fp16"][1] <= 0.5 * err["bf16"][1], err


class _Sub(torch.nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.c = torch.nn.Conv2d(cin, cout, 3, padding=1)
        self._pc = None

    def forward(self, t):
        from cwfa_amd import ops
        if self._pc is None or self._pc.epoch != ops.pack_epoch():
            self._pc = ops.pack_conv_weight(self.c.weight)
        return ops.conv2d(t, self._pc, bias=self.c.bias)


def _small_nets():
    from cwfa_amd import CWFA
    torch.manual_seed(0)
    np.random.seed(0)
    D, side, S = 16, 64, 3
    conv_inn, cond_nets = CWFA.build_networks(D, side, S, internal_chans=64, cond_chans=8, with_lrnn=False, device="cuda")
    g = torch.Generator().manual_seed(1)
    cond_input = torch.randn(1, 29, side, side, generator=g).cuda()
    mean = [0.1 * torch.randn(1, D // 2 ** (n + 1), side, side, generator=g).cuda() for n in range(S - 1)]
    low = torch.randn(1, D // 2 ** (S - 1), side, side, generator=g).cuda()
    return conv_inn, cond_nets, cond_input, mean, low


@pytest.mark.parametrize("prec", ["fp16", "split_bf16"])
def test_autocast_drop_in_inference(prec):
    """install(precision=...) and the installed modules under torch.autocast("cuda", float16) as CWFA.py:845 runs them: a CAT flow
    step (inverse and forward) and an AllInOneBlock with learned Householder reflections return bit-identical fp32 results inside and
    outside the region (the Householder product raised TypeError under autocast before)."""
    import cwfa_amd
    from cwfa_amd.FrEIA import modules as Fm
    cwfa_amd.install(precision=prec)
    conv_inn, cond_nets, cond_input, mean, low = _small_nets()
    g1 = conv_inn[1]

    def run():
        with torch.no_grad():
            c = [cond_nets[1](cond_input)[-1], mean[1]]
            up, _ = g1([torch.zeros((1,) + tuple(g1.global_out_shapes[0]), device="cuda"), low], c=c, rev=True)
            z, j = g1(up, c=c)
        torch.manual_seed(5)
        np.random.seed(5)                 # (the fixed permutation is drawn from numpy's RNG, as in the reference)
        blk = Fm.AllInOneBlock([(8, 32, 40)], dims_c=[(4, 32, 40)], subnet_constructor=_Sub, learned_householder_permutation=2).cuda()
        gx = torch.Generator().manual_seed(6)
        xa, ca = torch.randn(2, 8, 32, 40, generator=gx).cuda(), torch.randn(2, 4, 32, 40, generator=gx).cuda()
        with torch.no_grad():
            (ya,), ja = blk((xa,), c=(ca,))
            (yr,), jr = blk((ya,), c=(ca,), rev=True)
        return [up, z[0] if isinstance(z, (list, tuple)) else z, j, ya, ja, yr, jr]
    plain = run()
    with torch.autocast("cuda", dtype=torch.float16):
        amp = run()
    for i, (a, b) in enumerate(zip(plain, amp)):
        assert b.dtype == a.dtype == torch.float32 and torch.equal(a, b), i


def test_autocast_training_step_with_grad_scaler():
    """One training step of a CAT step with its condition net in the reference's pattern (autocast forward, GradScaler(4),
    scale().backward(), unscale_, step, update) in fp16.  The unscaled gradients are bit-identical to those of the same scaled
    backward without autocast (the region changes nothing), scaler.step updates the parameters, and the gradients are within
    L2-rel 5e-3 of the split_bf16 mode's.  Against an UNSCALED backward they are not bit-identical: the data-gradient convolutions
    run on fp16 operands too, and gradients below 2^-14 are fp16 subnormals, whose rounding a power-of-two scale does change (the
    underflow GradScaler exists for) -- that difference is bounded here as well."""
    import cwfa_amd
    conv_inn, cond_nets, cond_input, mean, low = _small_nets()
    g1, cn = conv_inn[1].train(), cond_nets[1].train()
    gx = torch.Generator().manual_seed(9)
    gt = torch.randn(1, 8, 64, 64, generator=gx).cuda()
    params = [p for p in list(g1.parameters()) + list(cn.parameters()) if p.requires_grad]

    def loss_fn():
        torch.manual_seed(11)             # the same dropout draws in every pass
        c = [cn(cond_input)[-1], mean[1]]
        up, _ = g1([torch.zeros((1,) + tuple(g1.global_out_shapes[0]), device="cuda"), low], c=c, rev=True)
        Z, ljd = g1(gt, c=c)
        nll = (0.5 * torch.norm(Z[0]) ** 2 - ljd.mean()) / up.numel()
        return F.mse_loss(gt, up) * 0.5 + nll * 0.5

    def grads(scale=1.0):
        for p in params:
            p.grad = None
        (loss_fn() * scale).backward()
        return [None if p.grad is None else p.grad.detach() / scale for p in params]

    def l2rel(ga, gb):
        pairs = [(a, b) for a, b in zip(ga, gb) if b is not None]
        num = sum(float((a.double() - b.double()).norm() ** 2) for a, b in pairs)
        return (num / sum(float(b.double().norm() ** 2) for _, b in pairs)) ** 0.5

    cwfa_amd.install(precision="fp16")
    with torch.no_grad():
        loss_fn()                         # data-dependent initialisation (ActNorm) on a first batch, before any compared pass
    for p in params:
        p.grad = None
    with torch.autocast("cuda", dtype=torch.float16):
        loss = loss_fn()
    assert loss.dtype == torch.float32
    scaler = torch.amp.GradScaler("cuda", init_scale=2. ** 2)
    opt = torch.optim.SGD(params, lr=1e-3)
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    g_amp = [None if p.grad is None else p.grad.clone() for p in params]
    before = [p.detach().clone() for p in params]
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 2. ** 2, "the scaler found an inf / NaN gradient"
    assert sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, params)) > 0, "scaler.step did not update the parameters"
    with torch.no_grad():
        for a, p in zip(before, params):
            p.copy_(a)
    cwfa_amd.install(precision="fp16")    # (re-packs the banks of the restored weights)
    assert sum(a is not None for a in g_amp) > 0
    g_s = grads(2. ** 2)
    for i, (a, b) in enumerate(zip(g_amp, g_s)):
        assert (a is None and b is None) or torch.equal(a, b), i
    g_plain = grads()
    cwfa_amd.install(precision="split_bf16")
    g_ref = grads()
    e_scale, e_ref = l2rel(g_amp, g_plain), l2rel(g_plain, g_ref)
    print(f"training step: gradient L2-rel, scaled vs unscaled (fp16) {e_scale:.3e}, fp16 vs split_bf16 {e_ref:.3e}")
    assert e_scale <= 5e-3 and e_ref <= 5e-3, (e_scale, e_ref)
