"""GPU (MI355X): the 256-channel tiling of csrc/conv_split3x3.hip (MPW = 4: one pass over the n-tiles per k-step, the A fragments
of all four m-tiles held, B fragments two n-tiles ahead, one staging register set per entry) against a float64 convolution.

Shapes are the smallest at which that loop can go wrong:
  * Cout 256 (one cout tile) and 512 (two; block order with the XCD map on and off -- 32 x 64 has the 8 spatial tiles the map needs);
  * Cin 16 (ONE chunk: the trailing steps of the all-zero odd chunk are skipped), 48 (three chunks: the staging set serves an even
    chunk, an odd one and an even one again), 64 (two full periods);
  * 8 x 32 (one tile) and 24 x 40 (partial tiles in both directions: stores past the border are dropped);
  * with and without the load-side affine, with and without the skip add (the ADD form of the kernel), PReLU epilogue with
    per-channel slopes (the instantiations the UNet launches);
  * six products (split_bf16) and one product (bf16).
Bounds are those of tests/test_gpu_split_dispatch.py for this tiling: 5e-6 (max-rel and l2-rel) against float64 of the exact operands
in split precision; 2e-5 against float64 of the bf16-rounded operands in bf16 mode, the fp16 reference at least 10x further away.
Inputs have mixed signs and per-element magnitudes over 2^-3 .. 2^3, so a swapped or stale fragment cannot cancel."""
import itertools
import zlib

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from split_ref import _pro32, b16, check16, h, pack_split3x3

pytestmark = pytest.mark.gpu
SPLIT_TOL = 5e-6
COUT = 512                                   # the bank; the 256-output launches use its first 256 filters
B = 2
SHAPES = [(16, 8, 32), (48, 8, 32), (64, 8, 32), (16, 24, 40), (48, 24, 40), (64, 24, 40)]
PROS = [(aff, add) for aff in (False, True) for add in (False, True)]


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
    with torch.no_grad():
        yield
    ops.set_option("split3x3_xcd_map", 1)
    ops.set_precision("fp32")


_INPUTS, _REF = {}, {}


def inputs(cin, H, W):
    """Seeded CPU tensors of a shape.  x, sc, sh and add lie on a dyadic grid (multiples of 2^-4 below 8 in magnitude, sc in
    {0.5, 1, 2}): x * sc + sh + add is then exact in fp32 whether the kernel fuses it or rounds twice, so no element changes
    sides of a bf16 rounding boundary in one-product mode.  Weights: normal draws times 2^(-3 .. 3) per (filter, channel)."""
    key = (cin, H, W)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))

        def dy(*s):
            return torch.randint(-127, 128, s, generator=g).float() / 16

        w = torch.randn(COUT, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        w = w * 2.0 ** torch.randint(-3, 4, (COUT, cin, 1, 1), generator=g).float()
        _INPUTS[key] = {"x": dy(B, cin, H, W), "w": w, "b": torch.randn(COUT, generator=g),
                        "alpha": torch.randint(-4, 9, (COUT,), generator=g).float() / 8,
                        "sc": 2.0 ** torch.randint(-1, 2, (B, cin), generator=g).float(), "sh": dy(B, cin), "add": dy(B, cin, H, W)}
    return _INPUTS[key]


def reference(cin, H, W, aff, add, rnd):
    """float64: conv of the operands rounded by rnd (None: exact) + bias -> per-channel PReLU; all 512 filters, once"""
    key = (cin, H, W, aff, add, None if rnd is None else rnd.__name__)
    if key not in _REF:
        t = inputs(cin, H, W)
        r = rnd or (lambda v: v.double())
        xin = _pro32(t["x"], t["sc"] if aff else None, t["sh"] if aff else None, t["add"] if add else None)
        lin = F.conv2d(r(xin), r(t["w"]), padding=1) + t["b"].double().view(1, -1, 1, 1)
        _REF[key] = torch.where(lin > 0, lin, t["alpha"].double().view(1, -1, 1, 1) * lin)
    return _REF[key]


def check(fmt, got, shape, aff, add, cout, what):
    if fmt == "split_bf16":
        assert_close(got, reference(*shape, aff, add, None)[:, :cout], SPLIT_TOL, what)
    else:
        check16(got, reference(*shape, aff, add, b16)[:, :cout], reference(*shape, aff, add, h)[:, :cout], what)


def launch(ops, dev, cout, aff, add):
    return ops.conv2d(dev["x"], dev["pc"][cout], bias=dev["b"][:cout].contiguous(), act="prelu", prelu_alpha=dev["alpha"][:cout].contiguous(),
                      in_scale=dev["sc"] if aff else None, in_shift=dev["sh"] if aff else None, in_add=dev["add"] if add else None)


def on_device(ops, t):
    dev = {k: v.cuda() for k, v in t.items()}
    dev["pc"] = {cout: pack_split3x3(ops, dev["w"][:cout].contiguous()) for cout in (256, 512)}
    assert all(pc.split for pc in dev["pc"].values())
    return dev


@pytest.mark.parametrize("fmt", ("split_bf16", "bf16"))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"cin{c}_{H}x{W}" for c, H, W in SHAPES])
def test_onepass_vs_float64(shape, fmt):
    """256 and 512 outputs x (affine, skip add) of one shape in one operand format against float64; two cout tiles: the plain
    block order computes the same bits"""
    from cwfa_amd import ops
    ops.set_precision(fmt)
    t = inputs(*shape)
    dev = on_device(ops, t)
    for cout, (aff, add) in itertools.product((256, 512), PROS):
        what = f"cin {shape[0]} {shape[1]}x{shape[2]} cout {cout} aff {aff} add {add} {fmt}"
        y = launch(ops, dev, cout, aff, add)
        assert y.shape == (B, cout, shape[1], shape[2])
        check(fmt, y, shape, aff, add, cout, what)
        if cout == 512:
            ops.set_option("split3x3_xcd_map", 0)
            try:
                assert torch.equal(launch(ops, dev, cout, aff, add), y), (what, "split3x3_xcd_map 0")
            finally:
                ops.set_option("split3x3_xcd_map", 1)


@pytest.mark.parametrize("fmt", ("split_bf16", "bf16"))
def test_onepass_xcd_map_eight_tiles(fmt):
    """32 x 64 = 8 spatial tiles x 2 cout tiles: the XCD-aware block map really applies; on and off agree bit for bit and with float64"""
    from cwfa_amd import ops
    ops.set_precision(fmt)
    shape = (48, 32, 64)
    t = inputs(*shape)
    dev = on_device(ops, t)
    for aff, add in ((False, False), (True, True)):
        what = f"cin 48 32x64 cout 512 aff {aff} add {add} {fmt}"
        y = launch(ops, dev, 512, aff, add)
        check(fmt, y, shape, aff, add, 512, what)
        ops.set_option("split3x3_xcd_map", 0)
        try:
            assert torch.equal(launch(ops, dev, 512, aff, add), y), (what, "split3x3_xcd_map 0")
        finally:
            ops.set_option("split3x3_xcd_map", 1)
