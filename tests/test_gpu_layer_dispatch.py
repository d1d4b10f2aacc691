"""GPU (MI355X): every launch form of the fused split layer kernel (csrc/conv_split_layer.hip), bit-exactly.

layer_launch selects among 13 forms of split_layer_kernel<SIX, INB, OUTB, NPER, TAPE, XF, SHORT, F16> and builds each for the three
operand formats (six-product split, bf16, fp16): 39 instantiations.  layer_ref.select restates that selection; the case lists below
are asserted (at import) to reach all 13 x 3, so a form added later fails the import until it has a case.

a. test_exact_small: the integer data set of layer_ref (every operand an integer of <= 8 bits, both ELUs exact) at the smallest
   shapes at which each mechanism exists.  y -- and the hidden map of the tape form -- must equal float64 rounded to fp32 bit for bit.
   NCHW x and u are channel slices between NaN channels, a blocked x is a per-sample slab followed by a NaN pad, y and hid are slices
   of NaN-filled buffers whose outside must keep its NaN bits (batch strides never the dense one); the NCHW forms also run with
   every tensor one float past a 16-byte boundary; every sample alone is bit-equal to its slice of the batched launch.
b. test_exact_walk: the same data generated on the device at a geometry derived from the CU count (MI355X: 256 CUs -> 4 x 123 x 791,
   800 tiles, every workgroup walks 3 tiles and 32 walk 4, the XCD tile map on; second geometry 4 x 107 x 919, 812 tiles, unmapped):
   batch vs each sample alone (alone there is no walk), the last sample vs the float64 reference (computed once per geometry on the
   CPU), and the same bits with the option split3x3_xcd_map off.
c. test_random_*: rounding only (indexing is settled by a and b).  Equality chains leave three anchors per format -- plain
   (layouts 0 = 1 = 2 = 3 = tape y), first layer with x given (layouts 0 = 1 = 2 = 3), fused first map (XF 0 = XF 2 = SHORT 0 =
   SHORT 2).  Split format: 3e-6 (plain) and 5e-6 (first-layer forms) against float64.  bf16 / fp16 plain anchor: the tape hidden
   map by check16 at 2e-5 against float64 over operands rounded as the kernel rounds them, y by check16 against the 1x1 phase on the
   kernel's own hidden map.  fp16 first-layer anchors: 2.5e-4.  bf16 first-layer anchors: BF16_FIRST_TOL, twice the largest figure
   measured (below).
d. test_contract: every rejected call returns non-zero and leaves a NaN-filled y untouched; empty sizes return 0.

Every test prints its figure next to its bound before it asserts (pytest -s).  Largest figure measured on an MI355X (max-rel):
  split_bf16   plain y 3.3e-7, hidden map 8.6e-7 (3e-6); first layer with x given 1.8e-7, fused first map 2.3e-7 (5e-6)
  bf16         plain: hidden map 3.6e-7, y on the kernel's hidden map 8.4e-8 (2e-5), the fp16 reference >= 1.7e-3 away
               first layer: 7.9e-5 at (2,17,45), 1.652e-4 at (1,70,96), the same with x given and with the fused first map
               -> BF16_FIRST_TOL = 3.3e-4 = 2 x 1.652e-4 (a single rounding-boundary flip of one hidden element moves y by one bf16
               ulp of that element, so the figure depends on the seed); the fp16 reference is 2.07e-3 (x given) / 3.2e-3 (fused)
               away: 12.5 x the measured figure at the least, which is what check16 asks (it would not be 10 x the bound itself)
  fp16         plain: hidden map 3.1e-7, y 8.9e-8 (2e-5), the bf16 reference >= 1.5e-3 away; first layer 4.2e-5 (2.5e-4), the
               bf16 reference >= 2.1e-3 away
Parts a and b: 116 small cases and 26 walk cases in each of the three formats, all bit-equal to float64, no NaN neighbour read, nothing
stored outside y / hid, with the kernels as they stand: no kernel was changed.  Not covered here or anywhere: the grouped-launch
path of the kernel (nprob > 1, spp, MAXP), which no entry point reaches (all three pass nprob = 1).
"""
import ctypes as C
from dataclasses import dataclass

import pytest
import torch
import torch.nn.functional as F

import layer_ref as R
from conftest import assert_close, rel_err
from layer_ref import FORMATS, _from_blocked, _to_blocked
from split_ref import F16_TOL, b16, check16, h, maxrel

pytestmark = pytest.mark.gpu
NAN = float("nan")
NAN_BITS = int(torch.tensor([NAN]).view(torch.int32)[0])
PLAIN_TOL, FIRST_TOL, FP16_FIRST_TOL = 3e-6, 5e-6, 2.5e-4
BF16_FIRST_TOL = 3.3e-4             # twice the largest figure measured (module docstring)


# ------------------------------------------------------------------------------------------------ forms and cases
@dataclass(frozen=True)
class Form:
    name: str
    entry: str                        # "plain" | "tape" | "first"
    layout: int = 0                   # bit 0: x channel-blocked, bit 1: y channel-blocked
    x_none: bool = False              # first-layer entry point with x = NULL: the launch forms its first map itself (XF)
    short: bool = False               # layout | 4: the short packed image (u_ch <= 16)

    def key(self, u_ch=13):
        return R.select(self.entry, self.layout, self.x_none, self.short, hid=self.entry == "tape", u_ch=u_ch)


FORMS = ([Form(f"plain{l}", "plain", l) for l in range(4)] + [Form("tape", "tape")]
         + [Form(f"first{l}", "first", l) for l in range(4)]
         + [Form(f"xf{l}", "first", l, x_none=True) for l in (0, 2)]
         + [Form(f"short{l}", "first", l, x_none=True, short=True) for l in (0, 2)])
FORM = {f.name: f for f in FORMS}
SHAPES = [(1, 16, 32),                # one full tile
          (2, 17, 45),                # 2 x 2 ragged tiles, W % 4 != 0
          (1, 5, 3),                  # less than one wave row pair
          (3, 16, 17),                # one pixel into the second n-tile
          (1, 33, 64),                # one row into a third tile row
          (1, 31, 100),               # ragged fourth tile column
          (2, 1, 1)]                  # single pixel


@dataclass(frozen=True)
class Case:
    form: Form
    shape: tuple
    cin: int = 12                     # channels of u without the ones channel: u_ch = cin + 1
    mis: bool = False                 # x, u, y and hid each start one float past a 16-byte boundary

    @property
    def id(self):
        return f"{self.form.name}-{'x'.join(map(str, self.shape))}-c{self.cin}" + ("-mis" if self.mis else "")


def _small_cases():
    out = [Case(f, s) for f in FORMS for s in SHAPES]                          # cin = 12: short and long images both exist
    for f in FORMS:
        if f.entry == "first":
            # u_ch = 16: the SHORT limit; 17: just past it (the short bit is rejected there); 32: both chunks full
            out += [Case(f, SHAPES[1], cin) for cin in (15, 16, 31) if not (f.short and cin + 1 > 16)]
        if f.layout == 0:                                                      # the NCHW forms, off the 16-byte grid
            out.append(Case(f, SHAPES[1], mis=True))
    return out


SMALL = _small_cases()
WALK_FORMS = FORMS                    # part b: every form, both geometries, cin = 12
assert len({c.id for c in SMALL}) == len(SMALL)
# every form in parts a and b; every form at the first four shapes; every u_ch at (2,17,45); the short limit from both sides
assert {c.form.key(c.cin + 1) for c in SMALL} == R.ALL_FORMS and {f.key() for f in WALK_FORMS} == R.ALL_FORMS
assert len(FORMS) == 13 and len({f.key() for f in FORMS}) == 13 and len(FORMATS) == 3
assert len({(fmt, c.form.key(c.cin + 1)) for fmt in FORMATS for c in SMALL}) == 39 == len({(fmt, f.key()) for fmt in FORMATS for f in WALK_FORMS})
assert all({c.shape for c in SMALL if c.form == f} >= set(SHAPES[:4]) for f in FORMS)
assert all(any(c.cin == cin and c.shape == (2, 17, 45) and c.form == f for c in SMALL)
           for cin in (12, 15, 16, 31) for f in FORMS if f.entry == "first" and not (f.short and cin > 15))
assert R.select("first", 0, x_none=True, short=True, u_ch=16) is not None and R.select("first", 0, x_none=True, short=True, u_ch=17) is None
assert all(any(c.mis and c.form == f for c in SMALL) for f in FORMS if f.layout == 0)
assert all(c.form.key(c.cin + 1) is not None for c in SMALL)


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()
    _DATA.clear()
    _MAPS.clear()
    _WALK.clear()


@pytest.fixture(autouse=True)
def _restore():
    from cwfa_amd import ops
    with torch.no_grad():
        yield
    ops.set_option("split3x3_xcd_map", 1)
    ops.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ device layouts
def nan_around(shape, before, after, off=0):
    """a [B,C,H,W] view that is the channel slice [before, before + C) of a NaN-filled [B, before + C + after, H, W] tensor starting
    ``off`` floats into its (aligned) allocation; -> (view, whole allocation)"""
    B, Cc, H, W = shape
    n = B * (before + Cc + after) * H * W
    flat = torch.full((n + 4,), NAN, device="cuda")
    return flat[off:off + n].view(B, before + Cc + after, H, W)[:, before:before + Cc], flat


def nan_padded(B, n, pad=8):
    """a [B, n] view of per-sample slabs, each followed by ``pad`` NaN floats (a multiple of 4: every slab 16-byte aligned)"""
    flat = torch.full((B * (n + pad),), NAN, device="cuda")
    return flat.view(B, n + pad)[:, :n], flat


def untouched_outside(view, flat):
    """every element of the allocation outside the view still has the NaN bit pattern it was filled with"""
    probe = flat.clone()
    probe.as_strided(view.size(), view.stride(), view.storage_offset() - flat.storage_offset()).fill_(NAN)
    return bool((probe.view(torch.int32) == NAN_BITS).all())


def bits_equal(a, b):
    a, b = a.contiguous(), b.to(a.device).contiguous()
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


class Maps:
    """the inputs of a launch on the device: x as an NCHW view and as a channel-blocked [B, 64 HW] view, u1 = (u | 1)"""

    def __init__(self, x, xb, u1):
        self.x, self.xb, self.u1 = x, xb, u1
        self.B, _, self.H, self.W = x.shape

    @staticmethod
    def between_nans(x, u, mis=False):
        """x = channels 3:67 of 70, u1 a middle slice, the blocked x per-sample slabs with a NaN pad; every other element NaN"""
        B, _, H, W = x.shape
        u1 = torch.cat([u, torch.ones(B, 1, H, W, device=u.device)], 1).cuda()
        # (mis: the slices start a multiple of four channels in, so that the pointers are exactly one float past a 16-byte boundary)
        xs, _ = nan_around(tuple(x.shape), 4 if mis else 3, 2 if mis else 3, off=int(mis))
        xs.copy_(x)
        us, _ = nan_around(tuple(u1.shape), 4 if mis else 2, 3, off=int(mis))
        us.copy_(u1)
        xb, _ = nan_padded(B, 64 * H * W)
        xb.copy_(_to_blocked(x.cuda()).view(B, -1))
        assert xs.stride(0) == 70 * H * W and us.stride(0) != u1.shape[1] * H * W and xb.stride(0) % 4 == 0 and xb.data_ptr() % 16 == 0
        assert not mis or (xs.data_ptr() % 16 == 4 and us.data_ptr() % 16 == 4)
        return Maps(xs, xb, us)

    @staticmethod
    def dense(x, u):
        B, _, H, W = x.shape
        x = x.cuda()
        return Maps(x, _to_blocked(x).view(B, -1), torch.cat([u.cuda(), torch.ones(B, 1, H, W, device="cuda")], 1))


class Out:
    """an output map of a launch.  ``guard``: an NCHW map is the channel slice 3:67 (mis: 4:68) of a NaN-filled 69-channel tensor, a blocked one
    per-sample slabs with a NaN pad (batch stride never 64 HW); else dense"""

    def __init__(self, B, H, W, blocked, guard=True, mis=False):
        self.shape, self.blocked = (B, 64, H, W), blocked
        if not guard:
            self.flat = torch.empty(B * 64 * H * W, device="cuda")
            self.view = self.flat.view(B, 64 * H * W) if blocked else self.flat.view(B, 64, H, W)
        elif blocked:
            self.view, self.flat = nan_padded(B, 64 * H * W)
        else:
            self.view, self.flat = nan_around(self.shape, 4 if mis else 3, 1 if mis else 2, off=int(mis))
        self.guard = guard
        assert not guard or self.view.stride(0) != 64 * H * W

    def nchw(self):
        return _from_blocked(self.view.reshape(self.shape)) if self.blocked else self.view

    def clean_outside(self):
        return untouched_outside(self.view, self.flat)


def pack_layer(wt):
    """the packed image of the 64-channel layer in the active operand format, through the C entry point"""
    from cwfa_amd import _lib, ops
    L = _lib.lib()
    w3, w1 = wt["w3"].cuda().contiguous(), wt["w1"].cuda().contiguous()
    packed = torch.empty(L.cwfa_subnet_layer_split_packed_bytes(), dtype=torch.uint8, device="cuda")
    assert L.cwfa_subnet_layer_split_pack_f32(ops._p(w3), ops._p(w1), ops._p(packed), ops._stream()) == 0
    return packed


def pack_first(wt, short):
    """the composed image of the first-layer forms (ops.pack_first_layer_weight composes the banks)"""
    from cwfa_amd import ops
    pc = ops.pack_first_layer_weight(wt["w0"].cuda(), wt["b0"].cuda(), wt["w3"].cuda(), wt["w1"].cuda(), short=short)
    assert pc.short == short
    return pc.packed


class Banks:
    """the packed images and biases of one weight set in the active operand format"""

    def __init__(self, wt):
        self.wt, self.b3, self.b1, self._pk = wt, wt["b3"].cuda(), wt["b1"].cuda(), {}

    def packed(self, form):
        kind = "plain" if form.entry != "first" else "short" if form.short else "first"
        if kind not in self._pk:
            self._pk[kind] = pack_layer(self.wt) if kind == "plain" else pack_first(self.wt, form.short)
        return self._pk[kind]


def launch(form, m, bk, s=None, guard=True, mis=False):
    """one launch of a form over the whole batch of m, or over sample s alone, through the C entry point -> (y, hid or None)"""
    from cwfa_amd import _lib, ops
    L = _lib.lib()
    sl = slice(None) if s is None else slice(s, s + 1)
    B, H, W = (m.B if s is None else 1), m.H, m.W
    xin = (m.xb if form.layout & 1 else m.x)[sl]
    y = Out(B, H, W, bool(form.layout & 2), guard, mis)
    hid = Out(B, H, W, False, guard, mis) if form.entry == "tape" else None
    p, st = ops._p, ops._stream()
    if form.layout & 1:
        assert xin.data_ptr() % 16 == 0 and xin.stride(0) % 4 == 0
    if form.layout & 2:
        assert y.view.data_ptr() % 16 == 0 and y.view.stride(0) % 4 == 0
    if form.entry == "plain":
        rc = L.cwfa_subnet_layer_split_f32(p(xin), p(bk.packed(form)), p(bk.b3), p(bk.b1), p(y.view), B, H, W, xin.stride(0), y.view.stride(0),
                                           form.layout, st)
    elif form.entry == "tape":
        rc = L.cwfa_subnet_layer_split_tape_f32(p(xin), p(bk.packed(form)), p(bk.b3), p(bk.b1), p(y.view), p(hid.view), B, H, W, xin.stride(0),
                                                y.view.stride(0), hid.view.stride(0), st)
    else:
        u1 = m.u1[sl]
        rc = L.cwfa_subnet_layer_first_f32(p(u1), None if form.x_none else p(xin), p(bk.packed(form)), p(bk.b3), p(bk.b1), p(y.view), B,
                                           u1.shape[1], H, W, u1.stride(0), 0 if form.x_none else xin.stride(0), y.view.stride(0),
                                           form.layout | (4 if form.short else 0), st)
    assert rc == 0, (form.name, rc, L.cwfa_last_error())
    return y, hid


# ------------------------------------------------------------------------------------------------ a. exact, small
_DATA, _MAPS, _WALK = {}, {}, {}


def small_data(shape, cin):
    """the exact data set of a (shape, cin) with its float64 reference, once"""
    if (shape, cin) not in _DATA:
        _DATA[(shape, cin)] = R.exact_layer_data(*shape[:1], cin, *shape[1:], seed=1)
    return _DATA[(shape, cin)]


def small_maps(c):
    key = (c.shape, c.cin, c.mis)
    if key not in _MAPS:
        d = small_data(c.shape, c.cin)
        _MAPS[key] = Maps.between_nans(d["x"], d["u"], c.mis)
    return _MAPS[key]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("form", FORMS, ids=[f.name for f in FORMS])
def test_exact_small(form, fmt):
    """one form in one operand format at every small case of the form: the bits of float64, nothing read or written outside"""
    from cwfa_amd import ops
    ops.set_precision(fmt)
    banks = {}
    cases = [c for c in SMALL if c.form == form]
    for c in cases:
        d, m = small_data(c.shape, c.cin), small_maps(c)
        bk = banks.setdefault(c.cin, Banks(d["wt"]))
        y, hid = launch(form, m, bk, mis=c.mis)
        torch.cuda.synchronize()
        assert not c.mis or (y.view.data_ptr() % 16 == 4 and (hid is None or hid.view.data_ptr() % 16 == 4))
        for name, o, ref in (("y", y, d["ref"]["y"]), ("hid", hid, d["ref"]["hidden"])):
            if o is None:
                continue
            assert o.clean_outside(), (c.id, fmt, name, "a store outside the output slice")
            got = o.nchw()
            assert not bool(torch.isnan(got).any()), (c.id, fmt, name, "a NaN neighbour leaked into the output (or an element was not written)")
            nbad = int((got.cpu() != ref.float()).sum())
            assert bits_equal(got, ref.float()), (c.id, fmt, name, f"{nbad} elements differ from float64", maxrel(got, ref))
        for s in range(c.shape[0]):
            ys, hs = launch(form, m, bk, s=s, mis=c.mis)
            assert bits_equal(ys.nchw(), y.nchw()[s:s + 1]), (c.id, fmt, "sample", s)
            assert ys.clean_outside()
            if hid is not None:
                assert bits_equal(hs.nchw(), hid.nchw()[s:s + 1]) and hs.clean_outside(), (c.id, fmt, "hidden map of sample", s)
    print(f"exact {form.name} {fmt}: {len(cases)} cases bit-equal to float64")


# ------------------------------------------------------------------------------------------------ b. exact, persistent walk
def walk_data(second):
    """the exact data of a walk geometry, generated on the device; the float64 reference of the LAST sample, once per geometry"""
    if second not in _WALK:
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        B, H, W, T, total = R.walk_premises(n_cu, second)
        d = R.exact_layer_data(B, 12, H, W, seed=2 + int(second), device="cuda", ref_samples=slice(B - 1, B))
        _WALK[second] = (d, Maps.dense(d["x"], d["u"]), (n_cu, B, H, W, T, total))
    return _WALK[second]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("second", [False, True], ids=["mapped", "unmapped"])
@pytest.mark.parametrize("form", WALK_FORMS, ids=[f.name for f in WALK_FORMS])
def test_exact_walk(form, second, fmt):
    """more tiles than three times the CUs: every workgroup stages a next tile, carries the weight ring's phase over two tile
    boundaries and ends on the all-out-of-range staging of its last tile"""
    from cwfa_amd import ops
    d, m, (n_cu, B, H, W, T, total) = walk_data(second)
    xmap = total % 8 == 0 and min(total, n_cu) % 8 == 0
    assert xmap != second and total // n_cu >= 3 and T <= n_cu
    ops.set_precision(fmt)
    bk = Banks(d["wt"])
    y, hid = launch(form, m, bk, guard=False)
    outs = [("y", y.nchw(), d["ref"]["y"])] + ([("hid", hid.nchw(), d["ref"]["hidden"])] if hid is not None else [])
    for s in range(B):
        ys, hs = launch(form, m, bk, s=s, guard=False)
        assert bits_equal(ys.nchw(), outs[0][1][s:s + 1]), (form.name, fmt, "walk vs sample alone", s)
        if hid is not None:
            assert bits_equal(hs.nchw(), outs[1][1][s:s + 1]), (form.name, fmt, "hidden map, walk vs sample alone", s)
    for name, got, ref in outs:
        nbad = int((got[B - 1:].cpu() != ref.float()).sum())
        assert bits_equal(got[B - 1:], ref.float()), (form.name, fmt, name, f"{nbad} elements of the last sample differ from float64")
    if not second:
        try:
            ops.set_option("split3x3_xcd_map", 0)
            y0, hid0 = launch(form, m, bk, guard=False)
        finally:
            ops.set_option("split3x3_xcd_map", 1)
        assert bits_equal(y0.nchw(), outs[0][1]), (form.name, fmt, "without the XCD tile map")
        assert hid is None or bits_equal(hid0.nchw(), outs[1][1])
    print(f"walk {form.name} {fmt}: {B} x {H} x {W}, {total} tiles on {n_cu} CUs, tile map {'on' if xmap else 'off'}: bit-equal")


# ------------------------------------------------------------------------------------------------ c. random data: rounding
RANDOM_SHAPES = [(2, 17, 45), (1, 70, 96)]
RANDOM_CIN = 12                       # the short form exists
_RANDOM = {}


def random_data(shape):
    if shape not in _RANDOM:
        B, H, W = shape
        cin = RANDOM_CIN
        g = torch.Generator().manual_seed(H * W + 17)
        t = {"xp": torch.randn(B, 64, H, W, generator=g), "u": torch.randn(B, cin, H, W, generator=g),
             "w0": torch.randn(64, cin, 1, 1, generator=g) / cin ** 0.5, "b0": torch.randn(64, generator=g) * 0.3,
             "w3": torch.randn(64, 64, 3, 3, generator=g) / 24, "b3": torch.randn(64, generator=g) * 0.1,
             "w1": torch.randn(64, 64, 1, 1, generator=g) / 8, "b1": torch.randn(64, generator=g) * 0.1}
        t["x"] = F.conv2d(t["u"], t["w0"], t["b0"])                      # the residual of the first-layer forms, when it is given (fp32)
        t["u1"] = torch.cat([t["u"], torch.ones(B, 1, H, W)], 1)
        t["w3c"], t["w0c"] = R.compose_first_layer(t["w0"], t["b0"], t["w3"])
        t["w3c"], t["w0c"] = t["w3c"][:, :cin + 1], t["w0c"][:, :cin + 1]
        _RANDOM[shape] = t
    return _RANDOM[shape]


def _chain(forms, m, bk):
    """launch the forms; all outputs bit-equal to the first -> (y, hid) of the first"""
    first, fh = None, None
    for f in forms:
        y, hid = launch(FORM[f], m, bk, guard=False)
        if first is None:
            first = y.nchw()
        else:
            assert bits_equal(y.nchw(), first), (f, "differs from", forms[0])
        fh = hid.nchw() if hid is not None else fh
    return first, fh


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_random_plain(shape, fmt):
    """plain layouts 0 = 1 = 2 = 3 = tape y; the anchor against float64"""
    from cwfa_amd import ops
    t = random_data(shape)
    ops.set_precision(fmt)
    bk = Banks(t)
    y, hid = _chain(["plain0", "plain1", "plain2", "plain3", "tape"], Maps.dense(t["xp"], t["u"]), bk)
    x, w3, b3, w1, b1 = t["xp"], t["w3"], t["b3"], t["w1"], t["b1"]

    def ref(rnd, hidden=None):
        hd = F.elu(F.conv2d(rnd(x), rnd(w3), b3.double(), padding=1))
        return F.elu(F.conv2d(rnd(hd.float() if hidden is None else hidden), rnd(w1), b1.double()) + x.double()), hd
    if fmt == "split_bf16":
        hr = F.elu(F.conv2d(x.double(), w3.double(), b3.double(), padding=1))
        yr = F.elu(F.conv2d(hr, w1.double(), b1.double()) + x.double())
        print(f"maxrel plain {fmt} {shape}: y {rel_err(y, yr)[0]:.3e}, hidden {rel_err(hid, hr)[0]:.3e}, bound {PLAIN_TOL:g}")
        assert_close(y, yr, PLAIN_TOL, "plain layer")
        assert_close(hid, hr, PLAIN_TOL, "hidden map of the tape form")
        return
    own, other = (b16, h) if fmt == "bf16" else (h, b16)
    hk = hid.cpu()
    print(f"maxrel plain {fmt} {shape}: hidden {maxrel(hid, ref(own)[1]):.3e} (other format {maxrel(hid, ref(other)[1]):.3e}), "
          f"y on the kernel's hidden map {maxrel(y, ref(own, hk)[0]):.3e} (other format {maxrel(y, ref(other, hk)[0]):.3e}), bound {F16_TOL:g}")
    check16(hid, ref(own)[1], ref(other)[1], f"hidden map of the tape form {fmt} {shape}")
    # the 1x1 phase against the kernel's own fp32 hidden map, rounded (a float64 hidden map rounds to another neighbour wherever the
    # fp32 accumulation error straddles a rounding boundary)
    check16(y, ref(own, hk)[0], ref(other, hk)[0], f"fused layer {fmt} {shape}")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("anchor", ["first", "xf"])
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_random_first(shape, anchor, fmt):
    """first layer, x given: layouts 0 = 1 = 2 = 3; fused first map: XF 0 = XF 2 = SHORT 0 = SHORT 2; the anchors against float64"""
    from cwfa_amd import ops
    t = random_data(shape)
    ops.set_precision(fmt)
    bk = Banks(t)
    fused = anchor == "xf"
    names = ["xf0", "xf2", "short0", "short2"] if fused else ["first0", "first1", "first2", "first3"]
    y, _ = _chain(names, Maps.dense(t["x"], t["u"]), bk)
    u, u1, w0, b0, w3, b3, w1, b1 = (t[k] for k in ("u", "u1", "w0", "b0", "w3", "b3", "w1", "b1"))
    if fmt == "split_bf16":                                    # the two convolutions evaluated one after the other
        x64 = F.conv2d(u.double(), w0.double(), b0.double())
        yr = F.elu(F.conv2d(F.elu(F.conv2d(x64, w3.double(), b3.double(), padding=1)), w1.double(), b1.double()) + x64)
        print(f"maxrel {anchor} {fmt} {shape}: {rel_err(y, yr)[0]:.3e}, bound {FIRST_TOL:g}")
        assert_close(y, yr, FIRST_TOL, f"composed first layer, {anchor}")
        return

    def ref(rnd):
        """float64 over rounded operands: the composed weights are what is rounded, the hidden map is rounded from the reference's
        own fp32 value"""
        hd = F.elu(F.conv2d(rnd(u1), rnd(t["w3c"]), b3.double(), padding=1))
        xr = F.conv2d(rnd(u1), rnd(t["w0c"]).reshape(64, -1, 1, 1)) if fused else t["x"].double()
        return F.elu(F.conv2d(rnd(hd.float()), rnd(w1), b1.double()) + xr)
    own, other = (b16, h) if fmt == "bf16" else (h, b16)
    e_own, e_other = maxrel(y, ref(own)), maxrel(y, ref(other))
    tol = FP16_FIRST_TOL if fmt == "fp16" else BF16_FIRST_TOL
    print(f"maxrel {anchor} {fmt} {shape}: {e_own:.3e} (other format {e_other:.3e}), bound {tol}")
    assert tol is not None, "BF16_FIRST_TOL has not been set from a measurement"
    check16(y, ref(own), ref(other), f"composed first layer, {anchor}, {fmt}, {shape}", tol=tol)


# ------------------------------------------------------------------------------------------------ d. contract
def test_contract():
    """every rejected call returns non-zero and leaves y untouched; an empty problem returns 0 and leaves y untouched"""
    from cwfa_amd import _lib, ops
    L = _lib.lib()
    ops.set_precision("split_bf16")
    B, H, W = 2, 8, 32
    n = 64 * H * W
    d = small_data((2, 17, 45), 15)
    bk = Banks(d["wt"])
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * n + 4, generator=g).cuda()
    u = torch.randn(B * 33 * H * W, generator=g).cuda()
    yf = torch.full((B * n + 4,), NAN, device="cuda")
    hf = torch.full((B * n + 4,), NAN, device="cuda")
    p, st = ops._p, ops._stream()
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)    # noqa: E731
    plain, first, short = (bk.packed(FORM[k]) for k in ("plain0", "first0", "short0"))
    b3, b1 = p(bk.b3), p(bk.b1)

    def split(xp, yp, layout, x_bs=n, y_bs=n, B=B, H=H, W=W):
        return L.cwfa_subnet_layer_split_f32(xp, p(plain), b3, b1, yp, B, H, W, x_bs, y_bs, layout, st)

    def tape(xp, yp, hp, B=B, H=H, W=W):
        return L.cwfa_subnet_layer_split_tape_f32(xp, p(plain), b3, b1, yp, hp, B, H, W, n, n, n, st)

    def frst(up, xp, yp, layout, u_ch=16, pk=first, y_bs=n, B=B, H=H, W=W):
        return L.cwfa_subnet_layer_first_f32(up, xp, p(pk), b3, b1, yp, B, u_ch, H, W, 33 * H * W, n, y_bs, layout, st)

    rejected = {
        "layout -1": lambda: split(P(x), P(yf), -1),
        "layout 8": lambda: split(P(x), P(yf), 8),
        "layout 8, first-layer entry point": lambda: frst(P(u), None, P(yf), 8, pk=short),
        "short bit with x": lambda: frst(P(u), P(x), P(yf), 4, pk=short),
        "short bit on the plain entry point": lambda: split(P(x), P(yf), 4),
        "short bit with u_ch = 17": lambda: frst(P(u), None, P(yf), 4, u_ch=17, pk=short),
        "u_ch = 0": lambda: frst(P(u), P(x), P(yf), 0, u_ch=0),
        "u_ch = 33": lambda: frst(P(u), P(x), P(yf), 0, u_ch=33),
        "u = NULL": lambda: frst(None, P(x), P(yf), 0),
        "blocked x off the 16-byte grid": lambda: split(P(x, 1), P(yf), 1),
        "blocked y off the 16-byte grid": lambda: split(P(x), P(yf, 1), 2),
        "blocked x_bs % 4": lambda: split(P(x), P(yf), 1, x_bs=n + 2),
        "blocked y_bs % 4": lambda: split(P(x), P(yf), 2, y_bs=n + 2),
        "blocked residual off the 16-byte grid": lambda: frst(P(u), P(x, 1), P(yf), 1),
        "blocked first-layer output, y_bs % 4": lambda: frst(P(u), None, P(yf), 2, y_bs=n + 2),
        "x == y": lambda: split(P(yf), P(yf), 0),
        "u == y": lambda: frst(P(yf), P(x), P(yf), 0),
        "hid == x": lambda: tape(P(x), P(yf), P(x)),
        "hid == y": lambda: tape(P(x), P(yf), P(yf)),
        "tape without a hidden map": lambda: tape(P(x), P(yf), None),
        "x = NULL on the plain entry point": lambda: split(None, P(yf), 0),
    }
    for what, call in rejected.items():
        assert call() != 0, (what, "was accepted")
        assert L.cwfa_last_error(), what
    # the calls above are accepted once their one fault is mended (each was rejected for the reason named)
    assert split(P(x), P(hf), 7 & 3) == 0 and frst(P(u), None, P(hf), 4, pk=short) == 0 and frst(P(u), None, P(hf), 2, u_ch=17) == 0
    for kw in ({"B": 0}, {"H": 0}, {"W": 0}):
        assert split(P(x), P(yf), 0, **kw) == 0 and split(P(x), P(yf), 3, **kw) == 0, kw
        assert tape(P(x), P(yf), P(hf[:1]), **kw) == 0 and tape(P(x), P(yf), None, **kw) == 0, kw
        assert frst(P(u), P(x), P(yf), 0, **kw) == 0 and frst(P(u), None, P(yf), 6, pk=short, **kw) == 0, kw
    torch.cuda.synchronize()
    assert bool((yf.view(torch.int32) == NAN_BITS).all()), "a rejected or empty call wrote y"
    assert not bool(torch.isnan(hf[:B * n]).any())
