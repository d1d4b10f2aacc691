"""GPU (MI355X): every launch form of the fused Conv3d forward (ops.conv3d_1k1) against float64.

csrc/conv3d.hip and csrc/conv3d_split.hip pick among six device paths:
  * cwfa_conv3d_1k1_f32, K <= 32: conv3d_1k1_mfma_kernel; K > 32: conv3d_1k1_kernel<6> (D % 6 == 0) or <8>;
  * cwfa_conv3d_1k1_split_f32 (K <= 32): conv3d_split_kernel<SIX, F16> in the formats split_bf16, bf16 and fp16, each with an interior
    and an edge block form, over a depth chunk DC from a cost loop, the accumulator ring walked in phases 0 / 1 / 2.
`conv3d_ref.dispatch` restates that selection and `conv3d_ref.CASES` is the case list; tests/test_conv3d_ref_cpu.py asserts, without
a GPU, what the list reaches: the three fp32 kernels, the split kernel in the three formats with DC = D for D = 1, 2, 3, DC = 4 with
a last chunk of 1, 2 and 3 slabs, DC = 5 and 6 (alone, under a batch, with interior blocks), chunks ending in each ring phase in both
block forms, interior blocks and edge blocks through H alone, W alone and both, H < 14 and W < 30, K = 1, 3, 17, 32 and 33, 40, 64, the
five PReLU slopes 0.25, -0.5, 0, 1, 1.5.

The C entry points are called directly.  Every case runs with
  * x and y inside flat device buffers filled with NaN, at least two H x W planes of NaN before and after each; in some cases x, y or
    both start one float past a 16-byte boundary;
  * the guard floats around y keeping their NaN bit pattern, and y finite everywhere (a guard NaN that was read and used shows even
    through a zero weight);
  * for B = 2, each sample launched alone (from NaN guards of its own) bit-equal to its slice of the batched launch;
  * a second launch giving the same bits.
Bounds:
  * fp32 MFMA, direct<6>, direct<8>, split_bf16: conftest.assert_close at 5e-6 against conv3d_ref64 (the project's bound);
  * fp16 / bf16: split_ref.check16 against conv3d_ref64 over operands and hidden map rounded to the format, fp16 at the project's
    2.5e-4, bf16 at 5e-6 (conv3d_ref.inputs makes the bf16 hidden map exact in fp32, so no hidden value can round to the
    neighbouring bf16; conv3d_ref.BF16_TOL has the argument), the other format's reference at least 4 bounds (and 10 errors) away;
    the one-voxel case cannot separate the formats (its references are 8e-6 apart) and is replaced by 1 x 1 x 9 x 20 there;
  * six-product sensitivity (conv3d_ref.py has the construction): on all-positive operands of which one carries a large third bf16
    piece, the split_bf16 kernel stays within TOL_PIECE = twice the fp32 MFMA kernel's measured error of the float64 result, while
    zeroing that third piece moves the float64 result by S >= 4 TOL_PIECE (asserted on the CPU): five products would fail;
  * K = 33 on the split entry point is the shape error, x == y the invalid-argument error, B, D, H or W = 0 is OK; none writes.

Every test prints its max-rel and l2-rel error next to the bound before it asserts (pytest -s).  Largest max-rel figure measured on
an MI355X, per kernel and format:
  fp32 MFMA     3.4e-7 (1x9x33x65_k32; bound 5e-6)
  direct<6>     1.9e-6 (1x12x17x40_k64), direct<8> 1.6e-6 (1x17x20x35_k64) (5e-6)
  split_bf16    4.1e-7 (1x13x30x62_k17; 5e-6)
  bf16          1.7e-7 (1x9x33x65_k32; 5e-6), the fp16 reference >= 1.75e-3 away
  fp16          5.6e-5 (1x9x33x65_k32; 2.5e-4), the bf16 reference >= 1.75e-3 away
  six products  fp32 MFMA 1.49e-7 .. 1.82e-7, hence tol_piece 2.97e-7 .. 3.65e-7; split_bf16 1.56e-7 .. 1.98e-7; the signal S
                5.58e-6 .. 6.02e-6 (>= 15 tol_piece), and the split result 5.6e-6 .. 6.1e-6 from the result without the third piece
On operands drawn as normal deviates (the first measurement; the l2-rel figures stayed near 1e-5) the bf16 format reached 4.7e-4 on
1x20x112x240_k32 and 2.9e-4 on 2x10x99x211_k17 through hidden values that round to the neighbouring bf16, with the fp16 reference
2.4e-3 .. 5.3e-3 away: four times that error is not four times below that distance, which is why inputs() bounds the operands'
dynamic range instead.  fp16 was 7.7e-5 at the most there.
All six paths passed every check -- bounds, NaN guards, finiteness, batch slices, repeatability -- as they stand: no kernel was changed."""
import pytest
import torch

import conv3d_ref as R
from conftest import assert_close, rel_err
from split_ref import b16, check16, h, maxrel

pytestmark = pytest.mark.gpu
NAN = float("nan")
NAN_BITS = int(torch.tensor([NAN]).view(torch.int32)[0])
OK, E_INVAL, E_SHAPE = 0, -1, -2


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
    ops.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ guarded buffers and launches
def guarded(shape, off=0, fill=None):
    """a contiguous view of `shape` inside a NaN-filled flat buffer: two H x W planes + 64 floats of NaN before and after it, the
    view `off` floats past a 16-byte boundary; -> (view, whole allocation)"""
    n = 1
    for s in shape:
        n *= s
    pad = (2 * shape[-2] * shape[-1] + 64 + 3) // 4 * 4
    flat = torch.full((pad + off + n + pad,), NAN, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[pad + off:pad + off + n].view(shape)
    assert view.data_ptr() % 16 == 4 * off
    if fill is not None:
        view.copy_(fill)
    return view, flat


def guards_untouched(view, flat):
    """every float of the allocation outside the view still has the NaN bit pattern it was filled with"""
    probe = flat.clone()
    start = view.storage_offset() - flat.storage_offset()
    probe[start:start + view.numel()] = NAN
    return bool((probe.view(torch.int32) == NAN_BITS).all())


def entry(fmt):
    """the C entry point of a precision (and, for the split kernel, its operand format made the active one)"""
    from cwfa_amd import _lib, ops
    ops.set_precision(fmt)
    L = _lib.lib()
    return L.cwfa_conv3d_1k1_f32 if fmt == "fp32" else L.cwfa_conv3d_1k1_split_f32


def launch(fn, x, wts, y, K):
    from cwfa_amd import ops
    B, D, H, W = x.shape
    w1, b1, a, w2, b2 = wts
    return fn(ops._p(x), ops._p(w1), ops._p(b1), ops._p(a), ops._p(w2), ops._p(b2), ops._p(y), B, D, H, W, K, ops._stream())


def run_guarded(fn, xs, wts, K, offx, offy, what):
    """one launch from / into NaN-guarded buffers; the guard, finiteness and repeatability checks; -> y (a fresh tensor)"""
    x, _ = guarded(tuple(xs.shape), offx, xs)
    y, yflat = guarded(tuple(xs.shape), offy)
    assert launch(fn, x, wts, y, K) == OK, what
    torch.cuda.synchronize()
    assert guards_untouched(y, yflat), (what, "a store outside y")
    assert bool(torch.isfinite(y).all()), (what, "y is not finite: a guard NaN was read and used, or a voxel was not written")
    first = y.clone()
    y.fill_(NAN)
    assert launch(fn, x, wts, y, K) == OK, what
    assert torch.equal(y, first), (what, "two launches differ")
    return first


def run_case(c, fmt):
    """the batched launch and, for B = 2, each sample alone bit-equal to its slice"""
    t = R.inputs(c)
    xs, wts = t[0].cuda(), [v.cuda().contiguous() for v in t[1:]]
    fn = entry(fmt)
    y = run_guarded(fn, xs, wts, c.K, c.offx, c.offy, (c.name, fmt))
    for s in range(c.B if c.B > 1 else 0):
        ys = run_guarded(fn, xs[s:s + 1], wts, c.K, c.offx, c.offy, (c.name, fmt, "sample", s))
        assert torch.equal(ys, y[s:s + 1]), (c.name, fmt, "sample", s, "alone differs from its slice of the batched launch")
    return y


def check64(c, fmt, y):
    ref = R.reference(c)
    m, l2 = rel_err(y, ref)
    print(f"conv3d {R.dispatch(*c.shape, c.K, fmt).kernel} {c.name}: max-rel {m:.3e}, l2-rel {l2:.3e}, bound {R.FP32_TOL:g}")
    assert_close(y, ref, R.FP32_TOL, f"{c.name} {fmt}")


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_fp32_entry_vs_float64(c):
    """cwfa_conv3d_1k1_f32: the MFMA kernel (K <= 32) and the direct kernels <6> / <8> (K > 32)"""
    assert R.dispatch(*c.shape, c.K, "fp32").kernel == ("mfma" if c.K <= 32 else "direct<6>" if c.D % 6 == 0 else "direct<8>")
    check64(c, "fp32", run_case(c, "fp32"))


@pytest.mark.parametrize("c,fmt", R.SPLIT_RUNS, ids=[f"{c.name}-{f}" for c, f in R.SPLIT_RUNS])
def test_split_entry_vs_float64(c, fmt):
    """cwfa_conv3d_1k1_split_f32 in one operand format: split_bf16 under the fp32 bound, bf16 / fp16 against the reference over
    operands and hidden map rounded as the kernel rounds them, the other format's reference clearly further away"""
    d = R.dispatch(*c.shape, c.K, fmt)
    assert d.kernel == f"split<{fmt}>"
    y = run_case(c, fmt)
    if fmt == "split_bf16":
        check64(c, fmt, y)
        return
    own, other, tol = (b16, h, R.BF16_TOL) if fmt == "bf16" else (h, b16, R.FP16_TOL)
    ref, ref_other = R.reference(c, own), R.reference(c, other)
    m, l2 = rel_err(y, ref)
    e_other = maxrel(y, ref_other)
    print(f"conv3d {d.kernel} {c.name} DC {d.DC}: max-rel {m:.3e}, l2-rel {l2:.3e}, bound {tol:g}; other format's reference {e_other:.3e}")
    check16(y, ref, ref_other, f"{c.name} {fmt}", tol=tol)
    assert l2 <= tol, (c.name, fmt, "l2-rel", l2)
    assert e_other >= 4 * tol, (c.name, fmt, "the bound does not separate the two formats", e_other, tol)


@pytest.mark.parametrize("shape", R.SENS_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("which", R.SENS_TENSORS)
def test_split_keeps_all_six_products(which, shape):
    """the split_bf16 kernel within TOL_PIECE of float64 where a dropped third piece of `which` is S >= 4 TOL_PIECE away; the fp32 MFMA
    kernel, whose measured error TOL_PIECE is twice of, is run beside it and held to the same figure"""
    key = R.sens_name(which, shape)
    t = R.sens_inputs(which, shape)
    full, drop, S = R.sens_refs(which, shape)
    xs, wts = t[0].cuda(), [v.cuda().contiguous() for v in t[1:]]
    y32 = run_guarded(entry("fp32"), xs, wts, R.SENS_K, 0, 0, (key, "fp32"))
    ysp = run_guarded(entry("split_bf16"), xs, wts, R.SENS_K, 0, 0, (key, "split_bf16"))
    tol = R.TOL_PIECE.get(key, 0.0)
    (m32, l32), (msp, lsp) = rel_err(y32, full), rel_err(ysp, full)
    print(f"conv3d six products {key}: signal S {S:.3e}; fp32 MFMA max-rel {m32:.3e}, l2-rel {l32:.3e}; split_bf16 max-rel {msp:.3e}, "
          f"l2-rel {lsp:.3e} (from the result without the third piece: {maxrel(ysp, drop):.3e}); bound tol_piece {tol:.3e}")
    assert S >= 4 * tol > 0, (key, S, tol)
    assert_close(y32, full, tol, f"{key} fp32 MFMA")
    assert_close(ysp, full, tol, f"{key} split_bf16")


def _all_nan(t):
    torch.cuda.synchronize()
    return bool((t.view(torch.int32) == NAN_BITS).all())


def test_rejected_and_empty_calls_write_nothing():
    from cwfa_amd import _lib, ops
    L = _lib.lib()
    g = torch.Generator().manual_seed(7)
    B, D, H, W = 2, 5, 9, 33
    x = torch.randn(B, D, H, W, generator=g).cuda()
    y = torch.full((B, D, H, W), NAN, device="cuda")

    def wts(K):
        return [v.cuda() for v in (torch.randn(K, 1, 3, 3, 3, generator=g), torch.randn(K, generator=g), torch.tensor([0.25]),
                                   torch.randn(1, K, 3, 3, 3, generator=g), torch.randn(1, generator=g))]
    w32, w33 = wts(32), wts(33)
    for fmt in R.FORMATS:
        ops.set_precision(fmt)
        assert launch(L.cwfa_conv3d_1k1_split_f32, x, w33, y, 33) == E_SHAPE, fmt          # K <= 32 only
        assert launch(L.cwfa_conv3d_1k1_split_f32, x, w32, x, 32) == E_INVAL, fmt          # in place
    ops.set_precision("fp32")
    for K, w in ((32, w32), (33, w33)):
        assert launch(L.cwfa_conv3d_1k1_f32, x, w, x, K) == E_INVAL
    assert _all_nan(y) and bool(torch.isfinite(x).all())
    for shp in ((0, D, H, W), (B, 0, H, W), (B, D, 0, W), (B, D, H, 0)):
        for fn, K, w in ((L.cwfa_conv3d_1k1_f32, 32, w32), (L.cwfa_conv3d_1k1_f32, 33, w33), (L.cwfa_conv3d_1k1_split_f32, 32, w32)):
            rc = fn(ops._p(x), ops._p(w[0]), ops._p(w[1]), ops._p(w[2]), ops._p(w[3]), ops._p(w[4]), ops._p(y), *shp, K, ops._stream())
            assert rc == OK, (shp, K)
    assert _all_nan(y), "an empty problem wrote its output"
