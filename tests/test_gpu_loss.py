"""GPU (MI355X): the weighted-MSE loss `wL2` -- the fused pass cwfa_wmse_loss_f32 through ops.wmse_loss and
losses.weighted_mse_loss against the fixtures g23_wmse* (the reference's own losses.weighted_mse_loss with torch autograd on the CPU,
in fp32 and in float64: tools/make_loss_golden.py), and the manual training path with loss_func="wL2" against torch.autograd over the
reference's expression on the installed modules."""
import ctypes

import pytest
import torch

import loss_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
CASES = ["odd_tail", "two_samples", "blocks_and_tail", "constant_pred", "ths_zero", "disjoint"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def table():
    return R.load()


def _cu(a):
    return torch.from_numpy(a).cuda()


def _check_sums(out, c, what):
    """out = (sum, count) of the kernel against the fixture: the count exactly, sum / numel against the float64 loss within four times
    the error of the reference's own fp32 result (measured by the generator, stored in the fixture)."""
    n = c["gt"].size
    got, want, bound = float(out[0]) / n, float(c["loss64"]), 4.0 * float(c["ref32_err"])
    print(f"{what}: count {int(out[1])} (stored {int(c['count32'])}), loss {got!r}, float64 {want!r}, |diff| {abs(got - want):.3e}, "
          f"bound {bound:.3e}")
    assert float(out[1]) == int(c["count32"]), f"{what}: in-mask count"
    assert abs(got - want) <= bound, f"{what}: loss off by {abs(got - want):.3e} > {bound:.3e}"


@pytest.mark.parametrize("name", CASES)
def test_ops_wmse_loss_against_the_reference(table, name):
    from cwfa_amd import ops
    c = table[name]
    gt, pred, n = _cu(c["gt"]), _cu(c["pred"]), c["gt"].size
    out, grad = ops.wmse_loss(gt, pred, c["ths_perc"], gscale=1.0 / n)
    assert out.dtype == torch.float64 and tuple(out.shape) == (2,) and grad.dtype == torch.float32 and grad.shape == gt.shape
    _check_sums(out.cpu(), c, name)
    R.check_grad(grad.cpu().numpy(), c, what=name)
    # bitwise reproducible; the map is optional and does not change the sums; a caller's extrema row is taken as given
    out2, grad2 = ops.wmse_loss(gt, pred, c["ths_perc"], gscale=1.0 / n)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    out3, none = ops.wmse_loss(gt, pred, c["ths_perc"], want_grad=False)
    assert none is None and torch.equal(out, out3)
    ext = ops.global_extrema(gt, pred)
    assert [float(ext[k]) for k in (0, 1, 4, 5)] == [float(v) for v in (gt.min(), gt.max(), pred.min(), pred.max())]
    out4, grad4 = ops.wmse_loss(gt, pred, c["ths_perc"], gscale=1.0 / n, extrema=ext)
    assert torch.equal(out, out4) and torch.equal(grad, grad4)
    # the other argument order: the same masks and sum, the negated map
    out5, grad5 = ops.wmse_loss(pred, gt, c["ths_perc"], gscale=1.0 / n)
    assert torch.equal(out, out5) and torch.equal(grad5, -grad)


@pytest.mark.parametrize("name", ["odd_tail", "blocks_and_tail"])
def test_ops_wmse_loss_on_tensors_off_the_16_byte_grid(table, name):
    """Contiguous tensors that start 4 bytes past a 16-byte boundary take the element-by-element path: the same checks."""
    from cwfa_amd import ops
    c = table[name]
    n = c["gt"].size

    def shifted(a):
        buf = torch.empty(n + 1, dtype=torch.float32, device="cuda")
        v = buf[1:].view(a.shape)
        v.copy_(_cu(a))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    gt, pred = shifted(c["gt"]), shifted(c["pred"])
    out, grad = ops.wmse_loss(gt, pred, c["ths_perc"], gscale=1.0 / n)
    _check_sums(out.cpu(), c, name + " (unaligned)")
    R.check_grad(grad.cpu().numpy(), c, what=name + " (unaligned)")
    out2, _ = ops.wmse_loss(gt, _cu(c["pred"]), c["ths_perc"], want_grad=False)          # one aligned, one not
    _check_sums(out2.cpu(), c, name + " (mixed alignment)")


def test_ops_wmse_loss_refuses_bad_arguments_and_accepts_empty_ones():
    from cwfa_amd import _lib, ops
    L = _lib.lib()
    a = torch.ones(2, 3, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        ops.wmse_loss(a, torch.ones(3, 2, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        ops.wmse_loss(a, torch.ones(3, 2, device="cuda").t())
    with pytest.raises(TypeError):
        ops.wmse_loss(a, a.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wmse_loss(a, a.cpu())
    with pytest.raises(ValueError, match="extrema"):
        ops.wmse_loss(a, a, extrema=torch.zeros(4, device="cuda"))
    # the C entry: a null `out` is refused before anything is launched; n = 0 zeroes `out` and touches nothing else
    ext, ws = ops.global_extrema(a, a), torch.zeros(2, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())         # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.cwfa_wmse_loss_f32(p(a), p(a), p(ext), 0.05, 1.0, None, None, p(ws), a.numel(), stream) == -1
    assert b"null out" in L.cwfa_last_error()
    out = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    grad = torch.full((4,), 5.0, device="cuda")
    assert L.cwfa_wmse_loss_f32(None, None, None, 0.05, 1.0, p(grad), p(out), None, 0, stream) == 0
    assert out.tolist() == [0.0, 0.0] and grad.tolist() == [5.0] * 4
    e = torch.empty(0, 3, device="cuda")
    out, grad = ops.wmse_loss(e, e)
    assert out.tolist() == [0.0, 0.0] and grad.shape == e.shape


@pytest.mark.parametrize("name", CASES)
def test_losses_weighted_mse_loss_forward_and_backward(table, name):
    """The reference's signature: a 0-dim fp32 loss, `.backward()` into both arguments in both argument orders (with sign), the same
    value under no_grad, and a CPU tensor raises."""
    from cwfa_amd import losses, ops
    c = table[name]
    n = c["gt"].size
    out, _ = ops.wmse_loss(_cu(c["gt"]), _cu(c["pred"]), c["ths_perc"], want_grad=False)
    want = (out[0] / n).float()
    for first, second, sign in (("gt", "pred", 1.0), ("pred", "gt", -1.0)):
        a, b = _cu(c[first]).requires_grad_(), _cu(c[second]).requires_grad_()
        loss = losses.weighted_mse_loss(a, b, c["ths_perc"])
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad and torch.equal(loss, want)
        loss.backward()
        R.check_grad(a.grad.cpu().numpy(), c, sign=sign, what=f"{name}: d loss / d {first} (first argument)")
        R.check_grad(b.grad.cpu().numpy(), c, sign=-sign, what=f"{name}: d loss / d {second} (second argument)")
    # only the input that needs a gradient gets one; an upstream factor scales the map
    a, b = _cu(c["gt"]), _cu(c["pred"]).requires_grad_()
    (losses.weighted_mse_loss(a, b, c["ths_perc"]) * 0.5).backward()
    assert a.grad is None
    R.check_grad(2.0 * b.grad.cpu().numpy(), c, sign=-1.0, what=f"{name}: half the loss")
    asked, real = [], ops.wmse_loss
    ops.wmse_loss = lambda *args, **kw: (asked.append(kw["want_grad"]), real(*args, **kw))[1]
    try:
        with torch.no_grad():
            quiet = losses.weighted_mse_loss(_cu(c["gt"]), _cu(c["pred"]).requires_grad_(), c["ths_perc"])
    finally:
        ops.wmse_loss = real
    assert asked == [False], "under no_grad no gradient map is written"
    assert not quiet.requires_grad and torch.equal(quiet, want)
    if c["ths_perc"] == 0.05:
        assert torch.equal(losses.weighted_mse_loss(_cu(c["gt"]), _cu(c["pred"])), want)          # the default threshold
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.weighted_mse_loss(torch.from_numpy(c["gt"]), _cu(c["pred"]))


def _grads(mod):
    return {k: p.grad.clone() for k, p in mod.named_parameters() if p.grad is not None}


def _compare_grads(got, want, tol, what):
    assert set(got) == set(want) and len(want) > 40, (what, sorted(set(got) ^ set(want))[:6])
    errs = {k: max(rel_err(got[k], want[k])) for k in want}
    worst = max(errs, key=errs.get)
    print(f"{what}: worst relative gradient error {errs[worst]:.3e} ({worst}), bound {tol:g}")
    bad = [(k, e) for k, e in sorted(errs.items()) if not e <= tol]
    assert not bad, (what, bad[:6])


@pytest.mark.parametrize("gt_kind", ["fixture", "plateau"])
def test_step_backward_wl2_equals_autograd_over_the_reference_expression(gt_kind):
    """training.step_backward(loss_func="wL2") on the g13 CAT step against `full_loss.backward()` of the loss written as CWFA.py writes
    it (CWFA.py:952-987 with Losses.weighted_mse_loss(curr_gt, upsampled_vol), restated with torch operators) on the same modules.
    On the fixture's own ground truth (Gaussian) the gate leaves out a handful of elements only; "plateau" clamps it at its median,
    so that half of it sits at the minimum, outside the mask."""
    from cwfa_amd import training
    from test_gpu_autograd import _reference_loss, _step
    fx, g, _ = _step("g13_step_grad_k1_ch8")
    cu = lambda k: torch.from_numpy(fx[k]).cuda()       # noqa: E731
    w_c = 0.3
    c = [cu("c0").requires_grad_(), cu("c1").requires_grad_()]
    x = cu("x")
    if gt_kind == "plateau":
        x = torch.clamp(x, min=float(x.median())).contiguous()
    full, xhat, _ = _reference_loss(g, x, c, cu("full/z_in"), cu("full/low_in"), w_c, R.weighted_mse)
    mo, mt = R.masks(x, xhat.detach())
    share = float((mo & mt).float().mean())
    assert (share < 1.0) if gt_kind == "fixture" else (0.25 <= share <= 0.75), f"in-mask share {share}"
    full.backward()
    auto = _grads(g)
    for p in g.parameters():
        p.grad = None
    out = training.step_backward(g, x, [t.detach() for t in c], low=cu("full/low_in"), z=cu("full/z_in"), cond_weight=w_c,
                                 loss_func="wL2", want_cond_grads=True)
    print(f"in-mask share {share:.3f}, full_loss manual {float(out['full_loss'])!r}, autograd {float(full.detach())!r}")
    assert abs(float(out["full_loss"]) - float(full.detach())) <= 1e-5 * abs(float(full.detach()))
    assert abs(float(out["recon"]) - float(R.weighted_mse(x, xhat.detach()))) <= 1e-5 * abs(float(out["recon"]))
    _compare_grads(_grads(g), auto, 1e-4, "flow step, wL2: manual vs autograd")
    for k in (0, 1):
        m = max(rel_err(out["cond_grads"][k], c[k].grad))
        assert m <= 1e-4, (f"condition gradient {k}", m)
    with pytest.raises(NotImplementedError):
        training.step_backward(g, x, [t.detach() for t in c], low=cu("full/low_in"), z=cu("full/z_in"), loss_func="LL")


def test_lrnn_step_backward_wl2_equals_autograd_over_the_restated_loss():
    """training.lrnn_step_backward(loss_func="wL2") on the g11_lrnn_small network against torch.autograd over the restated loss on the
    LRNN's autograd nodes.  The target sits on a plateau at its minimum for about half of its elements, so the gate bites."""
    from cwfa_amd import networks as N, training
    from conftest import load_golden
    fs = load_golden("g11_lrnn_small")
    torch.manual_seed(int(fs["seed_init"]))
    enc = N.Encoder(29, 6, 5, 64, True)
    for m in enc.modules():
        if hasattr(m, "drop_out"):
            m.drop_out = 0                              # the dropout draws would differ between the two runs
    enc = enc.cuda().train()
    gi = torch.Generator().manual_seed(int(fs["seed_input"]))
    views = torch.randn(2, 29, 16, 16, generator=gi).cuda()
    noise = torch.randn(2, 6, 16, 16, generator=gi).cuda()
    out = enc(views)[-1]
    o = out.detach()
    gt = torch.clamp(o + 0.1 * o.std() * noise, min=float(o.median())).contiguous()
    mo, mt = R.masks(gt, o)
    share = float((mo & mt).float().mean())
    assert 0.25 <= share <= 0.75, share
    loss = R.weighted_mse(gt, out)
    loss.backward()
    auto = _grads(enc)
    for p in enc.parameters():
        p.grad = None
    for m in enc.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.reset_running_stats()
    loss2, out2 = training.lrnn_step_backward(enc, views, None, gt, loss_func="wL2")
    print(f"in-mask share {share:.3f}, loss manual {float(loss2)!r}, autograd {float(loss)!r}")
    assert abs(float(loss2) - float(loss)) <= 1e-5 * abs(float(loss))
    _compare_grads(_grads(enc), auto, 1e-4, "LRNN, wL2: manual vs autograd")
