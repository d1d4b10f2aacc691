"""GPU (MI355X): the persistent output convolution of csrc/conv_split_out.hip (64 -> Cout <= 48 channels, bias only) against float64.

Every launch goes through ops.conv2d, which must select the kernel (asserted): all three operand formats, every m-tile count and
ragged channel tail, both input layouts, ragged and exact tiles; more tiles than workgroups (the only way the next-tile staging and
the weight ring's hand-over from one tile to the next run) under both tile orders; and the store guards of an output that is a
channel slice.  References: float64 convolutions over the exact operands (split: 5e-6) or over operands rounded as the kernel rounds
them (bf16 / fp16: check16), one per (shape, rounding) for the widest bank -- narrower banks are its leading rows."""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from split_ref import b16, check16, h

pytestmark = pytest.mark.gpu
FORMATS = ("split_bf16", "bf16", "fp16")
SPLIT_TOL = 5e-6                          # the bound of test_gpu_split_dispatch.py
COUTS = (1, 12, 16, 17, 24, 33, 48)
SHAPES = ((1, 40, 72), (2, 16, 32))       # 3 x 3 tiles, ragged right and bottom; exactly one tile per sample
BIG = (2, 150, 430)                       # 10 x 14 x 2 = 280 tiles on at most 256 workgroups, both edges ragged
ROUND = {"split_bf16": None, "bf16": b16, "fp16": h}


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
    keep = ops.OUT_WALK, ops.OUT_WALK_MT
    ops.OUT_WALK, ops.OUT_WALK_MT = True, (1, 2, 3)        # every width, whatever the product's per-width decision
    with torch.no_grad():
        yield
    ops.OUT_WALK, ops.OUT_WALK_MT = keep
    ops.set_option("split3x3_xcd_map", 1)
    ops.set_precision("fp32")


_IN, _LIN = {}, {}


def inputs(shape):
    if shape not in _IN:
        g = torch.Generator().manual_seed(1000 * shape[1] + shape[2])
        B, H, W = shape
        _IN[shape] = (torch.randn(B, 64, H, W, generator=g), torch.randn(48, 64, 3, 3, generator=g) / 24.0, torch.randn(48, generator=g))
    return _IN[shape]


def reference(shape, fmt, cout):
    """float64 conv + bias of the operands as the format rounds them, for the leading ``cout`` rows of the 48-row bank"""
    key = (shape, fmt)
    if key not in _LIN:
        x, w, _ = inputs(shape)
        r = ROUND[fmt] or (lambda v: v.double())
        _LIN[key] = F.conv2d(r(x), r(w), padding=1)
    return _LIN[key][:, :cout] + inputs(shape)[2][:cout].double().view(1, -1, 1, 1)


def _to_blocked(t):
    B, Cc, H, W = t.shape
    return t.reshape(B, Cc // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().view(B, Cc, H, W)


def launch(ops, shape, cout, blocked=False, out=None, bias=True):
    """ops.conv2d on the bank's leading ``cout`` rows; NCHW input: a channel slice of a larger tensor (its own batch stride)"""
    x, w, b = inputs(shape)
    B, H, W = shape
    pc = ops.pack_conv_weight(w[:cout].contiguous().cuda())
    assert pc.walk is not None and ops.out_walk_selected(pc, H, W), "the bank did not select the persistent output convolution"
    if blocked:
        xd = _to_blocked(x.cuda())
    else:
        xb = torch.randn(B, 64 + 5, H, W).cuda()
        xb[:, 2:66] = x.cuda()
        xd = xb[:, 2:66]
    return ops.conv2d(xd, pc, bias=b[:cout].cuda() if bias else None, out=out, in_blocked=blocked), pc


def check(shape, fmt, cout, got, what):
    if fmt == "split_bf16":
        assert_close(got, reference(shape, fmt, cout), SPLIT_TOL, what)
    else:
        other = "fp16" if fmt == "bf16" else "bf16"
        check16(got, reference(shape, fmt, cout), reference(shape, other, cout), what)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cout", COUTS)
def test_formats_vs_float64(cout, fmt):
    from cwfa_amd import ops
    ops.set_precision(fmt)
    for shape in SHAPES:
        y, _ = launch(ops, shape, cout)
        check(shape, fmt, cout, y, f"Cout {cout} {fmt} {shape} NCHW")
        yb, _ = launch(ops, shape, cout, blocked=True)
        check(shape, fmt, cout, yb, f"Cout {cout} {fmt} {shape} blocked")
        assert torch.equal(y, yb), (cout, fmt, shape, "the input layout changed the arithmetic")


@pytest.mark.parametrize("xcd_map", (0, 1))
@pytest.mark.parametrize("cout", (12, 48))
def test_more_tiles_than_workgroups(cout, xcd_map):
    from cwfa_amd import ops
    ops.set_precision("split_bf16")
    assert torch.cuda.get_device_properties(0).multi_processor_count < 280
    ops.set_option("split3x3_xcd_map", xcd_map)
    try:
        y, _ = launch(ops, BIG, cout, blocked=True)
        torch.cuda.synchronize()
    finally:
        ops.set_option("split3x3_xcd_map", 1)
    check(BIG, "split_bf16", cout, y, f"Cout {cout} {BIG} xcd_map {xcd_map}")


@pytest.mark.parametrize("cout", (12, 17, 48))
def test_output_into_a_channel_slice(cout):
    """nothing outside the Cout planes is written: the zero rows that pad the bank to a multiple of 16 (Cout 12: rows 12 .. 15 would
    land in the four channels behind the slice) and ragged tiles' pixels outside the image leave nothing behind"""
    from cwfa_amd import ops
    ops.set_precision("split_bf16")
    shape = SHAPES[0]
    B, H, W = shape
    sentinel = -123456.75
    big = torch.full((B, cout + 6, H, W), sentinel, device="cuda")
    guard = big[:, cout:].clone()
    y, pc = launch(ops, shape, cout, out=big[:, :cout])
    assert y.data_ptr() == big.data_ptr()
    assert torch.equal(big[:, cout:].view(torch.int32), guard.view(torch.int32)), (cout, "a store behind the output slice")
    check(shape, "split_bf16", cout, big[:, :cout], f"Cout {cout} into a slice")
    # the packed image: [slice 18 x piece 3][k group 4][16 MT rows][16 bytes]; rows >= Cout are zeros
    rows = 16 * ((cout + 15) // 16)
    img = pc.walk.view(18 * 3, 4, rows, 16)
    assert pc.walk.numel() == 18 * 3 * 4 * rows * 16
    assert not bool(img[:, :, cout:].any()) and bool(img[:, :, :cout].any())
    # no bias = a zero bias
    y0, _ = launch(ops, shape, cout, bias=False)
    assert_close(y0, reference(shape, "split_bf16", cout) - inputs(shape)[2][:cout].double().view(1, -1, 1, 1), SPLIT_TOL, "no bias")
