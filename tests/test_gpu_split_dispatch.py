"""GPU (MI355X): every launch configuration of the split kernel of csrc/conv_split3x3.hip against float64.

The host code picks among 33 instantiations of conv3x3_split_kernel, (MPW, ADD, ACT1, KS, RPW, WM), and builds each for the three
operand formats (exact three-piece split, bf16, fp16): 99 kernels.  `dispatch` below restates that selection; the case list is
asserted to reach all 33 tuples, and every case runs in all three formats:
  * split_bf16: against float64 of the exact operands at 5e-6 (the bound of the other split tests);
  * bf16 / fp16: against float64 of the operands rounded as the kernel rounds them (RNE; bias, residual and epilogue in fp32)
    at max-rel 2e-5, with the other 16-bit format's reference at least 10x further away;
plus bit-level invariants (batch, writes past the Cout tail, block order, blocked layouts, 16-row tiles) and the contract of the
epilogue statistics: ops.conv_writes_stats is True exactly when a launch writes them, and they equal a pass over its output."""
import zlib
from dataclasses import dataclass

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from split_ref import F16_TOL, _pro32, b16, check16, h, maxrel, pack_split3x3, pack_split7x7

pytestmark = pytest.mark.gpu
FORMATS = ("split_bf16", "bf16", "fp16")
SPLIT_TOL = 5e-6
RUNTIME, COUPLE = -1, -2                  # the kernel's EPI_RUNTIME / EPI_COUPLE
ACT1 = {None: 0, "prelu": 2}              # compile-time epilogues (CWFA_ACT_NONE / CWFA_ACT_PRELU)


# ------------------------------------------------------------------------------------------------ the host selection, restated
def mpw_of(c):
    return 4 if c > 128 else 2 if c > 96 else 3 if c > 64 else 1 if c > 48 else 3 if c > 32 else 2 if c > 16 else 1


def wm_of(c):
    return 4 if c > 96 else 2 if c > 64 else 4 if c > 48 else 1


def _launch_epi(mpw, add, act, plain):
    if add:
        return (mpw, 1, 2 if plain and act == "prelu" else RUNTIME, 3, 4, 4)
    return (mpw, 0, ACT1[act] if plain and act in ACT1 else RUNTIME, 3, 4, 4)


def dispatch(c, rows16=True, special=False):
    """(MPW, ADD, ACT1, KS, RPW, WM) of the launch of case c; ``special``: out_stats or a blocked output is requested"""
    if c.kind == "couple":                                    # cwfa_conv3x3_split_couple_f32 (c.cout = n pairs)
        return (1, 0, COUPLE, 3, 8 if rows16 and c.H > 8 else 4, 4) if c.cout <= 32 else (2, 0, COUPLE, 3, 4, 4)
    if c.kind == "7x7":                                       # cwfa_conv7x7_split_f32
        return (2, 0, 0, 7, 4, 2)
    mpw, wm = mpw_of(c.cout), wm_of(c.cout)
    plain = not c.res and c.act2 is None
    if wm != 4:                                               # narrow tilings (ops.conv2d applies a prologue in a pass of its own)
        return (mpw, 0, ACT1[c.act] if plain and c.act in ACT1 else RUNTIME, 3, 8, wm)
    if mpw == 1 and rows16 and c.H > 8 and not c.pro:         # 64-channel tiling on 16-row tiles
        if plain and c.act is None:
            return (2, 0, 0, 3, 8, 2)
        if not special:
            return (2, 0, RUNTIME, 3, 8, 2)
    return _launch_epi(mpw, "add" in c.pro, c.act, plain)


def _epi5(mpw):
    return {(mpw, 0, 0, 3, 4, 4), (mpw, 0, 2, 3, 4, 4), (mpw, 0, RUNTIME, 3, 4, 4), (mpw, 1, 2, 3, 4, 4), (mpw, 1, RUNTIME, 3, 4, 4)}


TUPLES = (_epi5(4) | _epi5(2) | _epi5(1) | {(2, 0, 0, 3, 8, 2), (2, 0, RUNTIME, 3, 8, 2)}
          | {(m, 0, a, 3, 8, w) for m, w in ((3, 2), (3, 1), (2, 1), (1, 1)) for a in (0, 2, RUNTIME)}
          | {(1, 0, COUPLE, 3, 4, 4), (1, 0, COUPLE, 3, 8, 4), (2, 0, COUPLE, 3, 4, 4), (2, 0, 0, 7, 4, 2)})
assert len(TUPLES) == 33


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    cin: int
    cout: int                 # output channels (couple: pairs n)
    H: int
    W: int
    act: object = None        # act (couple: clamp kind)
    res: bool = False
    act2: object = None
    pro: str = ""             # load-side prologue: "aff" ([B,Cin] tables), "aff1" ([Cin] tables), "add" (skip tensor), combined by "+"
    pc: bool = True           # per-channel PReLU slopes
    kind: str = "3x3"         # "3x3" | "couple" | "7x7"
    rev: bool = False         # couple: inverse direction
    B: int = 2


CASES = [
    # launch_epi<4> (> 128 outputs)
    Case("e4_none", 17, 129, 9, 33, pro="aff"),
    Case("e4_prelu", 16, 257, 8, 31, act="prelu"),
    Case("e4_rt", 64, 160, 17, 20, act="elu", res=True, act2="gelu", pro="aff"),
    Case("e4_add_prelu", 3, 136, 1, 33, act="prelu", pro="aff+add"),
    Case("e4_add_rt", 33, 144, 9, 31, act="relu", res=True, act2="prelu", pro="add"),
    Case("e4_add_none", 16, 129, 8, 32, pro="add"),
    # launch_epi<2> (97 .. 128)
    Case("e2_none", 17, 97, 32, 40),                        # (8 spatial tiles: the XCD block map applies)
    Case("e2_prelu", 17, 128, 17, 31, act="prelu", pro="aff"),
    Case("e2_rt", 3, 112, 8, 33, act="gelu", res=True, act2="elu"),
    Case("e2_add_prelu", 16, 128, 9, 32, act="prelu", pro="add"),
    Case("e2_add_rt", 64, 104, 1, 31, act="prelu", act2="relu", pro="aff+add"),
    Case("e2_add_none", 33, 100, 17, 20, pro="add"),
    # launch_epi<1> (49 .. 64 with H <= 8 or a prologue)
    Case("e1_none", 33, 64, 17, 33, pro="aff"),
    Case("e1_prelu", 64, 49, 8, 31, act="prelu"),
    Case("e1_prelu_pt", 16, 64, 8, 32, act="prelu", pc=False),
    Case("e1_rt", 16, 56, 1, 32, act="elu", res=True),
    Case("e1_add_prelu", 17, 64, 9, 33, act="prelu", pro="aff1+add"),
    Case("e1_add_rt", 3, 50, 17, 31, res=True, act2="gelu", pro="add"),
    Case("e1_add_none", 64, 64, 8, 20, pro="add"),
    # 64-channel tiling on 16-row tiles (49 .. 64, H > 8, no prologue); 50 x 40: 8 spatial tiles (the XCD block map applies)
    Case("r16_none", 64, 64, 17, 40),
    Case("r16_none_xcd", 16, 49, 50, 40),
    Case("r16_prelu", 33, 64, 17, 33, act="prelu"),
    Case("r16_prelu_pt", 64, 50, 9, 33, act="prelu", pc=False),
    Case("r16_rt", 17, 60, 9, 31, act="gelu", res=True, act2="relu"),
    Case("r16_rt_b", 3, 64, 17, 20, act="relu", res=True, act2="elu"),
    # narrow tilings on 16-row tiles: (3, WM 2) 65 .. 96, (3, 1) 33 .. 48, (2, 1) 17 .. 32, (1, 1) <= 16
    Case("n96_none", 64, 65, 17, 32, pro="aff"),
    Case("n96_prelu", 17, 96, 9, 31, act="prelu"),
    Case("n96_rt", 3, 80, 1, 32, act="elu", res=True, act2="prelu"),
    Case("n48_none", 33, 33, 8, 33),
    Case("n48_prelu", 16, 48, 17, 31, act="prelu", pro="aff+add"),
    Case("n48_rt", 64, 40, 9, 20, act="prelu", res=True, act2="gelu"),
    Case("n32_none", 3, 17, 17, 33),
    Case("n32_prelu", 64, 32, 9, 31, act="prelu"),
    Case("n32_rt", 17, 24, 8, 31, act="gelu", res=True),
    Case("n16_none", 33, 16, 9, 33),
    Case("n16_prelu", 3, 7, 17, 20, act="prelu"),
    Case("n16_rt", 16, 16, 1, 33, act="relu", res=True, act2="relu"),
    # coupling epilogue (n pairs: 64 packed rows for n <= 32, on 16-row tiles when H > 8; 128 for n > 32)
    Case("cp_h8", 33, 24, 8, 33, act="ATAN", kind="couple"),
    Case("cp_r16", 16, 32, 17, 31, act="TANH", kind="couple", rev=True),
    Case("cp_n1", 3, 1, 9, 20, act="SIGMOID", kind="couple"),
    Case("cp_big", 64, 33, 9, 20, act="ATAN", kind="couple", rev=True),
    Case("cp_big64", 17, 64, 1, 33, act="NONE", kind="couple"),
    # 7x7 (<= 64 outputs)
    Case("k7_a", 17, 64, 9, 33, kind="7x7"),
    Case("k7_b", 33, 33, 8, 31, kind="7x7"),
]
IDS = [c.name for c in CASES]
assert len(set(IDS)) == len(IDS)
assert {dispatch(c) for c in CASES} == TUPLES, sorted(TUPLES - {dispatch(c) for c in CASES})
# every PReLU instantiation sees per-channel slopes; every activation of the run-time epilogue runs as act and as act2
assert all(any(c.pc and dispatch(c) == t for c in CASES if "prelu" in (c.act, c.act2)) for t in TUPLES if t[2] == 2)
assert all(any(c.act == a and c.res and dispatch(c)[2] == RUNTIME for c in CASES) and
           any(c.act2 == a and c.res and dispatch(c)[2] == RUNTIME for c in CASES) for a in ("elu", "prelu", "gelu", "relu"))


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _restore():
    from cwfa_amd import ops
    keep = ops.SPLIT_3X3_MIN_COUT, ops.SPLIT_3X3_NARROW_MAX
    with torch.no_grad():
        yield
    ops.SPLIT_3X3_MIN_COUT, ops.SPLIT_3X3_NARROW_MAX = keep
    ops.set_option("split3x3_xcd_map", 1)
    ops.set_option("split3x3_rows16", 1)
    ops.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ inputs and references
_INPUTS, _LIN = {}, {}


def inputs(c):
    """Seeded CPU tensors of a case.  With a load-side prologue x, sc, sh and add lie on a dyadic grid (multiples of 2^-4 below 8
    in magnitude, sc in {0.5, 1, 2}), so that x*sc + sh + add is exact in fp32 whether the kernel fuses it into one FMA or
    rounds twice as torch does: otherwise a rare element lands on the other side of a bf16 rounding boundary, and that one
    flip alone can exceed the 16-bit formats' bound.  The other inputs are plain normal draws."""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    B, ks = c.B, 7 if c.kind == "7x7" else 3
    rows = 2 * c.cout if c.kind == "couple" else c.cout

    def dy(*s):
        return torch.randint(-127, 128, s, generator=g).float() / 16

    t = {"x": dy(B, c.cin, c.H, c.W) if c.pro else torch.randn(B, c.cin, c.H, c.W, generator=g)}
    if c.kind == "couple":
        t["w"] = torch.randn(rows, c.cin, 3, 3, generator=g) * (1.5 / (3 * c.cin ** 0.5))
        t["b"] = torch.randn(rows, generator=g) * 0.1
        t["xh"] = torch.randn(B, c.cout, c.H, c.W, generator=g)           # the active half
    else:
        t["w"] = torch.randn(rows, c.cin, ks, ks, generator=g) / (c.cin * ks * ks) ** 0.5
        t["b"] = torch.randn(rows, generator=g)
    if c.res:
        t["res"] = torch.randn(B, c.cout, c.H, c.W, generator=g)
    if "prelu" in (c.act, c.act2):
        t["alpha"] = torch.randint(-4, 9, (c.cout,), generator=g).float() / 8 if c.pc else torch.tensor([0.25])
    if "aff" in c.pro:
        shp = (c.cin,) if "aff1" in c.pro else (B, c.cin)
        t["sc"] = 2.0 ** torch.randint(-1, 2, shp, generator=g).float()
        t["sh"] = dy(*shp)
    if "add" in c.pro:
        t["add"] = dy(B, c.cin, c.H, c.W)
    _INPUTS[c.name] = t
    return t


def linear(c, rnd):
    """float64 conv (no bias) of the operands rounded by rnd (None: exact), once per (case, rounding)"""
    key = (c.name, None if rnd is None else rnd.__name__)
    if key not in _LIN:
        t = inputs(c)
        r = rnd or (lambda v: v.double())
        xin = _pro32(t["x"], t.get("sc"), t.get("sh"), t.get("add"))       # fp32, exact (dyadic grid)
        _LIN[key] = F.conv2d(r(xin), r(t["w"]), padding=t["w"].shape[-1] // 2)
    return _LIN[key]


def _prelu(v, alpha):
    return torch.where(v > 0, v, alpha.double().view(1, -1, 1, 1) * v)


def _act(v, a, alpha):
    if a is None:
        return v
    return {"elu": F.elu, "gelu": F.gelu, "relu": F.relu}[a](v) if a != "prelu" else _prelu(v, alpha)


def reference(c, rnd):
    t = inputs(c)
    lin = linear(c, rnd) + t["b"].double().view(1, -1, 1, 1)
    if c.kind == "couple":
        n, clamp = c.cout, 1.7
        s = {"ATAN": lambda v: clamp * 0.636 * torch.atan(v), "TANH": lambda v: clamp * torch.tanh(v),
             "SIGMOID": lambda v: clamp * 2. * (torch.sigmoid(v) - 0.5), "NONE": lambda v: clamp * v}[c.act](lin[:, :n])
        tt, x = lin[:, n:], t["xh"].double()
        out = (x - tt) * torch.exp(-s) if c.rev else torch.exp(s) * x + tt
        return out, (-1 if c.rev else 1) * s.sum(dim=(1, 2, 3))
    v = _act(lin, c.act, t.get("alpha"))
    if c.res:
        v = v + t["res"].double()
    return _act(v, c.act2, t.get("alpha")), None


def check(c, fmt, got, what, ld=None):
    """the bound of the format (see the module docstring)"""
    if fmt == "split_bf16":
        ref, lref = reference(c, None)
        assert_close(got, ref, 1e-5 if c.kind == "couple" else SPLIT_TOL, f"{c.name} {what}")   # (couple: fast atan / tanh / exp)
    else:
        own, other = (b16, h) if fmt == "bf16" else (h, b16)
        ref, lref = reference(c, own)
        check16(got, ref, reference(c, other)[0], f"{c.name} {fmt} {what}")
    if ld is not None:
        assert maxrel(ld, lref) <= (1e-5 if fmt == "split_bf16" else F16_TOL), (c.name, fmt, what, "log-det", maxrel(ld, lref))


# ------------------------------------------------------------------------------------------------ launches
def _cu(t, key):
    return t[key].cuda() if key in t else None


class Dev:
    """the case's tensors on the device, in the layouts the launches read: x, the skip tensor and the residual as channel slices of
    larger tensors (input / residual / skip batch strides above their channel counts)"""

    def __init__(self, c):
        t = inputs(c)
        self.c, self.t = c, t
        B = c.B
        xb = torch.randn(B, c.cin + 5, c.H, c.W).cuda()
        xb[:, 2:2 + c.cin] = t["x"].cuda()
        self.x = xb[:, 2:2 + c.cin]
        self.w, self.b = t["w"].cuda(), t["b"].cuda()
        self.alpha, self.sc, self.sh = _cu(t, "alpha"), _cu(t, "sc"), _cu(t, "sh")
        self.res = self.add = None
        if "res" in t:
            rb = torch.randn(B, c.cout + 3, c.H, c.W).cuda()
            rb[:, 1:1 + c.cout] = t["res"].cuda()
            self.res = rb[:, 1:1 + c.cout]
        if "add" in t:
            ab = torch.randn(B, c.cin + 3, c.H, c.W).cuda()
            ab[:, 3:] = t["add"].cuda()
            self.add = ab[:, 3:]
        if "xh" in t:
            hb = torch.randn(B, c.cout + 4, c.H, c.W).cuda()
            hb[:, 4:] = t["xh"].cuda()
            self.xh = hb[:, 4:]

    def pack(self, ops):
        c = self.c
        if c.kind == "couple":
            self.bank = ops.pack_couple_weight(self.w, self.b)
            self.pc = self.bank[0]
        elif c.kind == "7x7":
            self.pc = pack_split7x7(ops, self.w)
            assert self.pc.ks == 7
        else:
            self.pc = pack_split3x3(ops, self.w)
        assert self.pc.split
        return self

    def run(self, ops, s=None, x=None, out=None, **kw):
        """one launch over the whole batch, or (s = sample index) over sample s alone; -> (output, log-det or None)"""
        c = self.c
        sl = slice(None) if s is None else slice(s, s + 1)
        x = self.x[sl] if x is None else x
        B = x.shape[0]
        if c.kind == "couple":
            if out is None:
                out = torch.empty(B, c.cout, c.H, c.W, device="cuda")
            ld = torch.zeros(B, dtype=torch.float64, device="cuda")
            ops.conv3x3_couple(x, self.bank, self.xh[sl], out, c.act, 1.7, 1.0, c.rev, logdet=ld, **kw)
            return out, ld
        sc = None if self.sc is None else self.sc if self.sc.dim() == 1 else self.sc[sl]
        sh = None if self.sh is None else self.sh if self.sh.dim() == 1 else self.sh[sl]
        y = ops.conv2d(x, self.pc, bias=self.b, act=c.act, prelu_alpha=self.alpha, residual=None if self.res is None else self.res[sl],
                       act2=c.act2, in_scale=sc, in_shift=sh, in_add=None if self.add is None else self.add[sl], out=out, **kw)
        return y, None

    def in_blocked_ok(self):
        # blocked input: Cin % 8 == 0, no skip tensor (and on the narrow tilings no prologue: ops.conv2d would apply it in an NCHW pass)
        c = self.c
        return c.kind != "7x7" and c.cin % 8 == 0 and "add" not in c.pro and not (c.kind == "3x3" and wm_of(c.cout) != 4 and c.pro)

    def out_blocked_ok(self):
        c = self.c
        return (c.kind == "3x3" and c.cout % 8 == 0 and wm_of(c.cout) == 4 and not c.res and c.act2 is None and c.act in ACT1
                and not ("add" in c.pro and c.act is None))


def _to_blocked(t):
    B, Cc, H, W = t.shape
    return t.reshape(B, Cc // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().view(B, Cc, H, W)


def _from_blocked(t):
    B, Cc, H, W = t.shape
    return t.reshape(B, Cc // 8, H, W, 8).permute(0, 1, 4, 2, 3).contiguous().view(B, Cc, H, W)


NAN_BITS = int(torch.tensor([float("nan")]).view(torch.int32)[0])


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_split_kernel_launch_vs_float64(c, fmt):
    """one launch configuration in one operand format: the float64 bound, then the bit-level invariants"""
    from cwfa_amd import ops
    ops.set_precision(fmt)
    d = Dev(c).pack(ops)
    # the output as a channel slice of a NaN-filled larger tensor: nothing past the Cout tail (nor before the slice) is written
    big = torch.full((c.B, c.cout + 5, c.H, c.W), float("nan"), device="cuda")
    y, ld = d.run(ops, out=big[:, 3:3 + c.cout])
    outside = torch.cat([big[:, :3], big[:, 3 + c.cout:]], 1)
    assert bool((outside.view(torch.int32) == NAN_BITS).all()), (c.name, fmt, "a store past the output channels")
    check(c, fmt, y, "", ld)
    y = y.clone()
    # batch: each sample alone == its slice of the batched launch
    for s in range(c.B):
        ys, lds = d.run(ops, s=s)
        assert torch.equal(ys, y[s:s + 1]), (c.name, fmt, "sample", s)
        if ld is not None:
            assert maxrel(lds, ld[s:s + 1]) <= 1e-12
    # block order: the XCD-aware block map and the plain one compute the same tiles
    ops.set_option("split3x3_xcd_map", 0)
    try:
        assert torch.equal(d.run(ops)[0], y), (c.name, fmt, "split3x3_xcd_map 0")
    finally:
        ops.set_option("split3x3_xcd_map", 1)
    # channel-blocked layouts: the same arithmetic, only the memory order differs
    if d.in_blocked_ok():
        assert torch.equal(d.run(ops, x=_to_blocked(d.x), in_blocked=True)[0], y), (c.name, fmt, "in_blocked")
    if d.out_blocked_ok():
        assert torch.equal(_from_blocked(d.run(ops, out_blocked=True)[0]), y), (c.name, fmt, "out_blocked")
    elif c.kind == "3x3" and c.cout % 8 == 0:
        with pytest.raises(ValueError):                       # (never an NCHW map where a blocked one was asked for)
            d.run(ops, out_blocked=True)
    # 16-row tiles off (the 64-channel tilings): the 8-row form is within the bound too
    if (c.kind == "3x3" and wm_of(c.cout) == 4 and mpw_of(c.cout) == 1) or (c.kind == "couple" and c.cout <= 32):
        ops.set_option("split3x3_rows16", 0)
        try:
            y8, ld8 = d.run(ops)
        finally:
            ops.set_option("split3x3_rows16", 1)
        check(c, fmt, y8, "rows16 off", ld8)


STATS_CASES = [c for c in CASES if c.kind != "couple"]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("c", STATS_CASES, ids=[c.name for c in STATS_CASES])
def test_epilogue_statistics_contract(c, fmt, monkeypatch):
    """out_stats: ops.conv_writes_stats is True exactly when the launch writes the statistics -- then they are (sum y, sum y^2) of
    the kernel's own y and y is bit-equal to the launch without them; otherwise ops.conv2d raises, and so does the C entry point
    when the request gets past ops (never a buffer left at zero)"""
    from cwfa_amd import _lib, ops
    ops.set_precision(fmt)
    d = Dev(c).pack(ops)
    writes = ops.conv_writes_stats(d.pc, c.act, d.res, c.act2, False, in_add=d.add is not None)
    st = torch.zeros(2 * c.cout, dtype=torch.float64, device="cuda")
    if not writes:
        with pytest.raises(ValueError):
            d.run(ops, out_stats=st)
        if c.kind == "3x3" and d.res is None and c.act2 is None and c.act in ACT1:
            monkeypatch.setattr(ops, "conv_writes_stats", lambda *a, **k: True)
            with pytest.raises(_lib.CwfaHipError, match=r"code -1\)"):          # CWFA_E_INVAL
                d.run(ops, out_stats=st)
            torch.cuda.synchronize()
            assert not bool(st.any())
        return
    y = d.run(ops, out_stats=st)[0]
    assert torch.equal(y, d.run(ops)[0]), (c.name, fmt, "y with and without out_stats")
    n = c.B * c.H * c.W
    ref64 = torch.stack([y.double().sum((0, 2, 3)), (y.double() ** 2).sum((0, 2, 3))], 1).cpu()
    got = st.cpu().view(-1, 2)
    scale = float(ref64[:, 1].max().sqrt()) * n ** 0.5          # |sum| <= sqrt(n * sumsq)
    assert float((got[:, 0] - ref64[:, 0]).abs().max()) <= 2e-6 * scale, (c.name, fmt, "sum y")
    assert float(((got[:, 1] - ref64[:, 1]) / ref64[:, 1]).abs().max()) <= 2e-6, (c.name, fmt, "sum y^2")
