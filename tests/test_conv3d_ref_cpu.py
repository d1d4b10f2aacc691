"""CPU: the restatement behind test_gpu_conv3d_dispatch.py (tests/conv3d_ref.py) -- conv3d_ref64 against torch's own Conv3d, what the
case list reaches through the restated host selection, and the pre-conditions of the six-product sensitivity cases."""
import pytest
import torch
import torch.nn.functional as F

import conv3d_ref as R
from split_ref import b16, h, maxrel


def _torch_conv3d(x, w1, b1, alpha, w2, b2, rnd=None):
    """the reference as test_fp16_conv3d states it"""
    r = rnd or (lambda t: t.double())
    v = r(x).permute(0, 2, 3, 1).unsqueeze(1)
    hid = F.prelu(F.conv3d(v, r(w1), b1.double(), padding=1), alpha.double())
    if rnd is not None:
        hid = rnd(hid.float())
    return F.conv3d(hid, r(w2), b2.double(), padding=1)[:, 0].permute(0, 3, 1, 2)


@pytest.mark.parametrize("cfg", [(2, 5, 7, 9, 3, 0.25), (1, 1, 2, 13, 5, -0.5), (1, 4, 1, 3, 2, 1.5)])
def test_restatement_equals_torch_conv3d(cfg):
    """biases of order 1: a hidden voxel outside the volume that is not zeroed is PReLU(b1 + ...) and shows in every border voxel"""
    B, D, H, W, K, alpha = cfg
    g = torch.Generator().manual_seed(D * H * W + K)
    x = torch.randn(B, D, H, W, generator=g)
    w1, b1 = torch.randn(K, 1, 3, 3, 3, generator=g) * 0.3, 1.0 + torch.rand(K, generator=g)
    w2, b2 = torch.randn(1, K, 3, 3, 3, generator=g) * 0.3, 1.0 + torch.rand(1, generator=g)
    a = torch.tensor([alpha])
    for rnd in (None, h, b16):
        got, want = R.conv3d_ref64(x, w1, b1, a, w2, b2, rnd), _torch_conv3d(x, w1, b1, a, w2, b2, rnd)
        assert tuple(got.shape) == (B, D, H, W) and got.dtype == torch.float64
        assert maxrel(got, want) <= 1e-14, (cfg, rnd, maxrel(got, want))
    # the border matters at these sizes: the same hidden map without its mask is far away
    hid = R.hidden_ref64(x, w1, b1, a)
    assert bool((hid[:, :, 0] == 0).all() and (hid[:, :, :, 0] == 0).all() and (hid[..., -1] == 0).all())


def test_dispatch_restates_the_anchors():
    d = R.dispatch(1, 20, 112, 240, 32, "split_bf16")
    assert (d.kernel, d.DC, d.chunks, d.interior) == ("split<split_bf16>", 5, ((5, 1),) * 4, True)
    d = R.dispatch(1, 9, 33, 65, 32, "bf16")
    assert (d.kernel, d.DC, d.chunks) == ("split<bf16>", 4, ((1, 0), (4, 0), (4, 0)))
    assert (d.interior, d.edge_h, d.edge_w, d.edge_hw) == (True, True, True, True)
    assert R.dispatch(1, 48, 512, 512, 32, "split_bf16").DC == 48          # 666 tiles: 3 rounds * 52 beats 8 * 20 (dc = 16) and 11 * 16 (dc = 12)
    assert R.dispatch(2, 3, 29, 31, 17, "fp16").DC == 3 and R.dispatch(1, 1, 1, 1, 1, "fp16").chunks == ((1, 0),)
    assert R.dispatch(1, 7, 5, 3, 3, "split_bf16").chunks == ((3, 2), (4, 0))
    assert R.dispatch(1, 6, 9, 33, 40, "fp32") == R.dispatch(1, 6, 9, 33, 40, "bf16") == R.Dispatch("direct<6>", DT=6)
    assert R.dispatch(1, 5, 9, 33, 33, "fp32").kernel == "direct<8>" and R.dispatch(1, 6, 9, 33, 32, "fp32").kernel == "mfma"


def test_case_list_reaches_every_launch_form():
    fp32 = [(c, R.dispatch(*c.shape, c.K, "fp32")) for c in R.CASES]
    assert {d.kernel for _, d in fp32} == {"mfma", "direct<6>", "direct<8>"}
    assert {c.K for c, d in fp32 if d.kernel == "mfma"} >= {1, 3, 17, 32}
    assert {c.K for c, d in fp32 if d.kernel.startswith("direct")} >= {33, 40, 64}
    for k in ("direct<6>", "direct<8>"):                       # one and several depth tiles, with and without a ragged last one
        sel = [c for c, d in fp32 if d.kernel == k]
        assert any(c.D <= d.DT for c, d in fp32 if d.kernel == k) and any(c.D > d.DT for c, d in fp32 if d.kernel == k), k
        assert sel
    assert any(c.D % 8 for c, d in fp32 if d.kernel == "direct<8>") and any(c.D % 8 == 0 for c, d in fp32 if d.kernel == "direct<8>")
    for fmt in R.FORMATS:
        sp = [(c, R.dispatch(*c.shape, c.K, f)) for c, f in R.SPLIT_RUNS if f == fmt]
        assert all(d.kernel == f"split<{fmt}>" for _, d in sp) and len(sp) >= len(R.MFMA_CASES) - 1
        assert {c.D for c, d in sp if d.DC == c.D and c.D < 4} == {1, 2, 3}
        assert {min(d.chunks)[0] for c, d in sp if d.DC == 4 and c.D % 4} == {1, 2, 3}     # DC = 4, last chunk of 1 / 2 / 3 slabs
        assert any(d.DC >= 5 for _, d in sp) and {d.DC for _, d in sp} >= {4, 5, 6}
        assert any(d.DC >= 5 and c.B == 2 for c, d in sp) and any(d.DC >= 5 and d.interior for c, d in sp)
        assert {ph for _, d in sp for _, ph in d.chunks} == {0, 1, 2}
        assert {ph for _, d in sp if d.interior for _, ph in d.chunks} == {0, 1, 2}         # ... and in the interior form
        assert any(d.interior for _, d in sp) and any(d.edge_h for _, d in sp) and any(d.edge_w for _, d in sp)
        assert all(d.edge_hw for _, d in sp)                   # (the first tile is always an edge block through both)
        assert any(c.H < R.SPLIT_HT and c.W < R.SPLIT_WT for c, _ in sp)
        assert {c.K for c, _ in sp} >= {1, 3, 17, 32}
    assert {c.alpha for c in R.CASES} == {0.25, -0.5, 0.0, 1.0, 1.5} == {c.alpha for c in R.MFMA_CASES} == {c.alpha for c in R.DIRECT_CASES}
    assert {(c.offx, c.offy) for c in R.MFMA_CASES} == {(0, 0), (1, 0), (0, 1), (1, 1)} == {(c.offx, c.offy) for c in R.DIRECT_CASES}
    assert any(c.B == 2 for c in R.MFMA_CASES) and any(c.B == 2 for c in R.DIRECT_CASES)


@pytest.mark.parametrize("c", [c for c in R.MFMA_CASES if c.B * c.D * c.H * c.W <= 30000], ids=lambda c: c.name)
def test_bf16_hidden_map_is_exact_in_fp32(c):
    """what conv3d_ref.inputs promises: over bf16 operands every product is a multiple of 2^-18 and b1 + their sum stays below 16, so
    the hidden value (times the slope) has at most 24 bits -- no order of fp32 accumulation can round it differently"""
    x, w1, b1, a, w2, b2 = R.inputs(c)
    assert bool((b16(x) * 2 ** 8 == (b16(x) * 2 ** 8).round()).all() and (b16(w1) * 2 ** 10 == (b16(w1) * 2 ** 10).round()).all())
    assert bool((b1.double() * 2 ** 10 == (b1.double() * 2 ** 10).round()).all())
    cols = R.hidden_ref64(b16(x).abs().float(), b16(w1).abs().float(), b1.abs(), torch.tensor([1.0]))     # the largest partial sum
    assert float(cols.max()) < 16
    hid = R.hidden_ref64(x, w1, b1, a, b16)
    assert bool((hid.float().double() == hid).all())
    assert float(b16(x).abs().min()) >= 0.5 and float(b16(w1).abs().min()) >= 0.125


def test_16bit_references_are_separable():
    """every case run in bf16 / fp16: the two rounded-operand references at least 5 bounds apart, so a result within one bound of
    its own reference is at least 4 bounds from the other's"""
    for c in R.MFMA_CASES:
        if c.fmt16:
            dist = maxrel(R.reference(c, b16), R.reference(c, h))
            assert dist >= 5 * max(R.BF16_TOL, R.FP16_TOL), (c.name, dist)
    assert sum(not c.fmt16 for c in R.MFMA_CASES) == 1


def test_piece_builders():
    g = torch.Generator().manual_seed(1)
    v = R.three_piece_values((4096,), g, -5)
    p0, p1, p2 = R.bf16_pieces(v)
    assert bool((v > 0).all() and (p0 > 0).all() and (p1 > 0).all() and (p2 > 0).all())
    assert bool((p0.double() + p1.double() + p2.double() == v.double()).all())
    for p in (p0, p1, p2):                                     # each piece is a bf16 value
        assert bool((p.bfloat16().float() == p).all())
    ratio = p2.double() / v.double()
    assert 1.3 * 2.0 ** -18 <= float(ratio.min()) and float(ratio.max()) <= 2.0 ** -17
    o = R.one_piece_values((4096,), g, 0)
    q0, q1, q2 = R.bf16_pieces(o)
    assert bool((q0 == o).all() and (q1 == 0).all() and (q2 == 0).all() and (o >= 1).all() and (o < 4).all())


@pytest.mark.parametrize("shape", R.SENS_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("which", R.SENS_TENSORS)
def test_sensitivity_preconditions(which, shape):
    """One tensor carries three pieces, the other two one; everything is positive; the float64 result moves by S when that tensor's
    third piece is zeroed, and S is at least four times the bound the split_bf16 kernel is held to on this case (TOL_PIECE: twice
    the fp32 MFMA kernel's measured error).  The hidden map has a third piece of its own in every case."""
    x, w1, b1, a, w2, b2 = t = R.sens_inputs(which, shape)
    assert float(a) == 1.0 and w1.shape[0] == R.SENS_K and tuple(x.shape) == shape
    for name, v in zip(("x", "w1", "b1", "w2", "b2"), (x, w1, b1, w2, b2)):
        p0, p1, p2 = R.bf16_pieces(v)
        assert bool((v > 0).all()), name
        if name == which:
            assert bool((p1 != 0).all() and (p2 != 0).all()), name
        else:
            assert bool((p1 == 0).all()), name
    hid = R.hidden_ref64(x, w1, b1, a)[:, :, 1:-1, 1:-1, 1:-1].float()
    assert float((R.bf16_pieces(hid)[2] != 0).double().mean()) > 0.5        # (a sum of 27 sixteen-bit products: 19 - 21 bits)
    d = R.dispatch(*shape, R.SENS_K, "split_bf16")
    assert d.DC == 4 and d.edge_hw and d.interior == (shape == R.SENS_SHAPES[1])
    full, drop, S = R.sens_refs(which, shape)
    tol = R.TOL_PIECE[R.sens_name(which, shape)]
    print(f"sensitivity {R.sens_name(which, shape)}: S {S:.3e}, tol_piece {tol:.3e}, S / tol_piece {S / tol:.1f}")
    assert 0 < tol and S >= 4 * tol, (which, shape, S, tol)
    assert tol < R.FP32_TOL                                    # (the case asks more than the general bound does)
