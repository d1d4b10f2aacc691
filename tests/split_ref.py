"""Helpers shared by the GPU tests of the split kernels (a plain module, not a conftest): float64 references over operands rounded
the way the kernels round them, and direct packing of filter banks that the selection rule of ops.pack_conv_weight would not send
to the split kernels."""
import torch

F16_TOL = 2e-5


def h(t):
    """fp16 operand as the kernels round it (torch's .half(): round to nearest even, +-inf beyond +-65504), in float64"""
    return t.half().double()


def b16(t):
    """bf16 operand as the kernels round it (round to nearest even), in float64"""
    return t.bfloat16().double()


def maxrel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max())


def check16(got, ref_own, ref_other, what, tol=F16_TOL):
    """the reference over operands in the format that should have run within tol; the other 16-bit format's reference at
    least 10x further away (the intended format really ran)"""
    e_own, e_other = maxrel(got, ref_own), maxrel(got, ref_other)
    assert e_own <= tol, (what, "vs the reference of its own operand format", e_own)
    assert e_other >= 10 * e_own, (what, "the other format's reference is not clearly further away", e_own, e_other)
    return e_own, e_other


def _pro32(x, sc=None, sh=None, add=None):
    """the kernels' load-side prologue in fp32: (x * sc + sh) + add; sc / sh are [C] or per-sample [B,C] tables"""
    v = x
    if sc is not None:
        lead = x.shape[0] if sc.numel() != x.shape[1] else 1
        v = v * sc.reshape(lead, -1, 1, 1) + sh.reshape(lead, -1, 1, 1)
    if add is not None:
        v = v + add
    return v


def pack_split3x3(ops, w):
    """The split 3x3 kernel's image of w [Cout,Cin,3,3] (on the device) in the active operand format, for every bank size:
    through ops.pack_conv_weight with the narrow tilings enabled for every bank with <= 32 outputs, and packed directly
    where the selection rule wants >= 29 inputs for them."""
    Cout, Cin = w.shape[:2]
    keep = ops.SPLIT_3X3_MIN_COUT, ops.SPLIT_3X3_NARROW_MAX
    ops.SPLIT_3X3_MIN_COUT, ops.SPLIT_3X3_NARROW_MAX = 1, 32
    try:
        if Cin >= 29 or Cout > 32:
            return ops.pack_conv_weight(w)
    finally:
        ops.SPLIT_3X3_MIN_COUT, ops.SPLIT_3X3_NARROW_MAX = keep
    L_ = ops._lib.lib()
    packed = torch.empty(L_.cwfa_conv3x3_split_packed_bytes(Cout, Cin), dtype=torch.uint8, device=w.device)
    wc = w.contiguous()
    ops.check(L_.cwfa_conv3x3_split_pack_f32(ops._p(wc), ops._p(packed), Cout, Cin, ops._stream()), "pack")
    return ops.PackedConv(packed, Cout, Cin, 3, False, wc._version, wc.data_ptr(), split=True)


def pack_split7x7(ops, w):
    """The split 7x7 kernel's image of w [Cout <= 64,Cin,7,7] (on the device); banks with < 32 inputs packed directly."""
    Cout, Cin = w.shape[:2]
    if Cin >= 32:
        return ops.pack_conv_weight(w)
    L_ = ops._lib.lib()
    packed = torch.empty(L_.cwfa_conv7x7_split_packed_bytes(Cout, Cin), dtype=torch.uint8, device=w.device)
    wc = w.contiguous()
    ops.check(L_.cwfa_conv7x7_split_pack_f32(ops._p(wc), ops._p(packed), Cout, Cin, ops._stream()), "pack 7x7")
    return ops.PackedConv(packed, Cout, Cin, 7, False, wc._version, wc.data_ptr(), split=True)
