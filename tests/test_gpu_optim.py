"""GPU: the fused Lion step (cwfa_lion_step_f32 behind cwfa_amd.optim.Lion) against tests/optim_ref.py, the float64 restatement of
the update rule.  Bounds (derived in optim_ref / DESIGN.md section 14, not measured): every output goes through at most four fp32
roundings, |m - m_ref| <= 4 * 2^-24 (|beta2 m0| + |(1 - beta2) g'|), |p - p_ref| <= 4 * 2^-24 (|p0| + lr); elements whose combination
beta1 m0 + (1 - beta1) g' is within rounding of zero are left out of the comparison of p, their share asserted <= 1e-5 per test
BEFORE anything is compared.  Every step is checked from the device's own fp32 state before that step."""
import numpy as np
import pytest
import torch

import optim_ref
from cwfa_amd import _lib
from cwfa_amd.optim import Lion

pytestmark = pytest.mark.gpu

MAXT, BLOCK = _lib.LION_MAX_TENSORS, _lib.LION_BLOCK_ELEMS
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2 * BLOCK + 3]


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()


def _state(opt):
    """Per group: (params with a gradient, their gradients, their exp_avg or zeros) as flat float32 arrays + the group's rates."""
    out = []
    for grp in opt.param_groups:
        ps = [p for p in grp["params"] if p.grad is not None]
        ms = [opt.state[p]["exp_avg"] if "exp_avg" in opt.state[p] else torch.zeros_like(p) for p in ps]
        out.append({"ps": ps, "p": _flat(ps), "g": _flat([p.grad for p in ps]), "m": _flat(ms), "lr": grp["lr"], "betas": grp["betas"],
                    "wd": grp["weight_decay"]})
    return out


def _step_and_check(opt, what, scale=None, step=None):
    """Run one step and compare every group against optim_ref from the state the device held before it."""
    before = _state(opt)
    (step or opt.step)()
    refs = [optim_ref.lion_step(b["p"], b["g"], b["m"], b["lr"], b["betas"], b["wd"], scale) for b in before]
    amb, tot = sum(int(r["ambiguous"].sum()) for r in refs), sum(b["p"].size for b in before)
    assert amb <= optim_ref.AMBIGUOUS_CAP * tot, f"{what}: {amb} of {tot} elements have a sign that rounding may decide"
    for k, (b, r) in enumerate(zip(before, refs)):
        assert np.array_equal(_flat([p.grad for p in b["ps"]]).view(np.uint32), b["g"].view(np.uint32)), f"{what}: a gradient was written"
        optim_ref.check(_flat(b["ps"]), _flat([opt.state[p]["exp_avg"] for p in b["ps"]]), r, f"{what}, group {k}")


def _params(sizes, gen, scale=1.0):
    return [torch.nn.Parameter((scale * torch.randn(n, generator=gen)).cuda()) for n in sizes]


def _set_grads(ps, gen, factor=1.0):
    for p in ps:
        p.grad = (factor * torch.randn(p.shape, generator=gen)).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("count", [MAXT - 1, MAXT, MAXT + 1, 2 * MAXT + 1])
def test_ragged_sizes_and_chunk_boundaries(count):
    """Tensors of 1 .. two-and-a-bit blocks mixed into lists around the chunk size of the argument table: three steps."""
    gen = torch.Generator().manual_seed(count)
    order = torch.randperm(count, generator=gen).tolist()
    ps = _params([SIZES[i % len(SIZES)] for i in order], gen)
    opt = Lion(ps, lr=1e-3, weight_decay=1e-2)
    for it in range(3):
        _set_grads(ps, gen)
        _step_and_check(opt, f"{count} tensors, step {it}")
    assert all(opt.state[p]["exp_avg"].shape == p.shape for p in ps)


def test_misaligned_views_take_the_scalar_path_and_leave_their_neighbours_alone():
    """Parameters, gradients and moments that are slices of flat buffers starting 1, 2, 3 floats past a 16-byte boundary, next to
    aligned ones: same check, and every float of the buffers outside the slices keeps its bits."""
    gen = torch.Generator().manual_seed(7)
    # (misalignment of p, of g, of m in floats; numel)
    plan = [(1, 0, 0, 5), (2, 2, 2, 1023), (3, 1, 0, BLOCK + 1), (0, 0, 0, 1025), (0, 3, 0, 4), (0, 0, 1, 2 * BLOCK + 3), (1, 1, 1, 1),
            (0, 0, 0, BLOCK), (3, 3, 3, 2 * BLOCK)]
    total = sum(n for *_, n in plan) + 16 * (len(plan) + 1)
    bufs = [torch.randn(total, generator=gen).cuda() for _ in range(3)]             # p, g, m
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    spans, cur = [], 8
    for rp, rg, rm, n in plan:
        base = (cur + 3) // 4 * 4
        spans.append(((base + rp, base + rg, base + rm), n))
        cur = base + 3 + n + 8
    ps = []
    opt_state = {}
    for (op, og, om), n in spans:
        p = torch.nn.Parameter(bufs[0][op:op + n])
        p.grad = bufs[1][og:og + n]
        opt_state[p] = bufs[2][om:om + n]
        assert p.data_ptr() == bufs[0].data_ptr() + 4 * op and p.is_contiguous()
        ps.append(p)
    opt = Lion(ps, lr=1e-3, weight_decay=1e-2)
    for p, m in opt_state.items():
        opt.state[p]["exp_avg"] = m
    outside = [torch.ones(total, dtype=torch.bool) for _ in range(3)]
    for offs, n in spans:
        for k in range(3):
            outside[k][offs[k]:offs[k] + n] = False
    for it in range(2):
        keep = [_bits(b) for b in bufs]
        _step_and_check(opt, f"misaligned views, step {it}")
        now = [_bits(b) for b in bufs]
        assert torch.equal(now[0][outside[0]], keep[0][outside[0]]), "floats around the parameter slices changed"
        assert torch.equal(now[2][outside[2]], keep[2][outside[2]]), "floats around the moment slices changed"
        assert torch.equal(now[1], keep[1]), "the gradient buffer changed"
        assert not torch.equal(now[0][~outside[0]], keep[0][~outside[0]])
        for p in ps:                                                                # fresh gradients in place: the views stay put
            p.grad.copy_(torch.randn(p.shape, generator=gen))


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("betas", [(0.9, 0.99), (0.5, 0.5)])
def test_hyper_parameters_and_two_groups(wd, betas):
    gen = torch.Generator().manual_seed(11)
    a, b = _params([1025, BLOCK + 7, 3], gen), _params([2 * BLOCK + 3, 5], gen, scale=3.0)
    opt = Lion([{"params": a, "weight_decay": wd}, {"params": b, "lr": 3e-5, "weight_decay": 0.1}], lr=1e-3, betas=betas)
    for it in range(2):
        _set_grads(a + b, gen)
        _step_and_check(opt, f"wd={wd} betas={betas}, step {it}")


def test_exact_cancellation_is_pure_decay():
    """beta1 = 0.5 and m0 = -g exactly: the combination is an exact zero, sign(0) = 0, and p = p0 * fp32(1 - fp32(lr * wd)) bit for bit."""
    gen = torch.Generator().manual_seed(13)
    ps = _params([1, 1025, BLOCK + 3], gen)
    _set_grads(ps, gen)
    lr, wd = 1e-3, 1e-2
    opt = Lion(ps, lr=lr, betas=(0.5, 0.99), weight_decay=wd)
    for p in ps:
        opt.state[p]["exp_avg"] = -p.grad.clone()
    F = np.float32
    decay = F(F(1) - F(F(lr) * F(wd)))
    assert decay != F(1)
    want = [torch.from_numpy(p.detach().cpu().numpy() * decay) for p in ps]
    m0 = [opt.state[p]["exp_avg"].clone() for p in ps]
    opt.step()
    for p, w, m in zip(ps, want, m0):
        assert torch.equal(_bits(p), _bits(w))
        ref = optim_ref.lion_step(np.zeros(p.numel(), F), _flat([p.grad]), _flat([m]), lr, (0.5, 0.99), wd)
        assert np.all(np.abs(_flat([opt.state[p]["exp_avg"]]) - ref["m"]) <= ref["m_tol"])


def test_parameters_without_a_gradient_are_left_alone():
    gen = torch.Generator().manual_seed(17)
    ps = _params([1025, 7, BLOCK + 5, 1024, 33], gen)
    frozen = ps[3]
    frozen.requires_grad_(False)
    opt = Lion(ps, lr=1e-3, weight_decay=1e-2)
    _set_grads([p for p in ps if p is not frozen], gen)
    _step_and_check(opt, "first step")                                              # ps[1] gets an exp_avg here
    ps[1].grad = None
    p_keep = {1: _bits(ps[1]), 3: _bits(frozen)}
    m_keep = _bits(opt.state[ps[1]]["exp_avg"])
    for it in range(2):
        _set_grads([ps[0], ps[2], ps[4]], gen)
        _step_and_check(opt, f"step {it} with a missing gradient")
        assert torch.equal(_bits(ps[1]), p_keep[1]) and torch.equal(_bits(frozen), p_keep[3])
        assert torch.equal(_bits(opt.state[ps[1]]["exp_avg"]), m_keep)
        assert "exp_avg" not in opt.state.get(frozen, {})
    from cwfa_amd import ops
    d = torch.zeros(4, dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        ops.lion_step([d], [d], [d], 1e-3, (0.9, 0.99), 0.0)


def _twins(gen, sizes):
    a = _params(sizes, gen)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    return a, b


def _same(opt_a, ps_a, opt_b, ps_b):
    for x, y in zip(ps_a, ps_b):
        if not torch.equal(_bits(x), _bits(y)) or not torch.equal(_bits(opt_a.state[x]["exp_avg"]), _bits(opt_b.state[y]["exp_avg"])):
            return False
    return True


def test_grad_scaler_unscales_and_skips_on_the_device():
    """GradScaler(init_scale=4) as CWFA.py:613.  A power-of-two scale makes the unscale exact: scaler.step(opt) on 4 g equals
    opt.step() on g bit for bit, with and without an explicit scaler.unscale_(opt); an inf or a NaN in ONE gradient leaves every
    parameter and every exp_avg as it was and halves the scale; the next clean step updates again."""
    gen = torch.Generator().manual_seed(19)
    sizes = [1025, 5, 2 * BLOCK + 3, 64]
    pa, pb = _twins(gen, sizes)
    oa, ob = Lion(pa, lr=1e-3, weight_decay=1e-2), Lion(pb, lr=1e-3, weight_decay=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=4.0)
    scaler.scale(torch.zeros((), device="cuda"))                                    # what `scaler.scale(loss)` does first: creates the scale

    def grads(poison=None):
        s = scaler.get_scale()
        for x, y in zip(pa, pb):
            x.grad = torch.randn(x.shape, generator=gen).cuda()
            y.grad = x.grad * s
        if poison is not None:
            pb[2].grad[BLOCK + 1] = poison

    grads()
    oa.step()
    _step_and_check(ob, "scaler.step on 4 g", scale=4.0, step=lambda: scaler.step(ob))
    scaler.update()
    assert not hasattr(ob, "grad_scale") and not hasattr(ob, "found_inf")
    assert _same(oa, pa, ob, pb), "scaler.step(opt) on 4 g differs from opt.step() on g"
    grads()
    oa.step()
    scaler.unscale_(ob)                                                              # the gradients are g again; the step gets no scale
    assert all(torch.equal(_bits(x.grad), _bits(y.grad)) for x, y in zip(pa, pb))
    _step_and_check(ob, "scaler.step after unscale_", step=lambda: scaler.step(ob))
    scaler.update()
    assert _same(oa, pa, ob, pb) and scaler.get_scale() == 4.0
    for poison, explicit_unscale in ((float("inf"), False), (float("nan"), False), (float("-inf"), True)):
        before = scaler.get_scale()
        grads(poison)
        keep = [(_bits(y), _bits(ob.state[y]["exp_avg"])) for y in pb]
        if explicit_unscale:
            scaler.unscale_(ob)
        scaler.step(ob)
        scaler.update()
        for y, (kp, km) in zip(pb, keep):
            assert torch.equal(_bits(y), kp) and torch.equal(_bits(ob.state[y]["exp_avg"]), km), f"a step with {poison} wrote something"
        assert scaler.get_scale() == before / 2
    assert _same(oa, pa, ob, pb)
    grads()                                                                          # scale 0.5 by now: still a power of two
    oa.step()
    _step_and_check(ob, "clean step after the skipped ones", scale=scaler.get_scale(), step=lambda: scaler.step(ob))
    scaler.update()
    assert _same(oa, pa, ob, pb)


def test_real_parameter_set_and_training_iteration():
    """A CAT flow step's parameters with the gradients of its training loss (fixture g13, as the gradient tests load it): one Lion step
    from m0 = 0 against optim_ref.  Then one whole training iteration of a small pyramid with make_optimizers and wd = 0: every
    parameter a gradient reached moves by exactly lr, against the sign of its gradient (from m0 = 0 exp_avg has that sign), every other
    one keeps its bits (the one parameter that two condition nets share takes a step in each of their optimisers)."""
    from cwfa_amd import CWFA, training
    from test_gpu_backward import _golden_step
    fx, g = _golden_step("g13_step_grad_k0_ch8")
    x = torch.from_numpy(fx["x"]).cuda()
    c = [torch.from_numpy(fx["c0"]).cuda(), torch.from_numpy(fx["c1"]).cuda()]
    training.step_backward(g, x, c, cond_weight=0.0)
    named = dict(g.named_parameters())
    assert {k for k, p in named.items() if p.grad is not None} == {k[len("grad/"):] for k in fx if k.startswith("grad/")}
    idle = {k: _bits(p) for k, p in named.items() if p.grad is None}
    opt = Lion(g.parameters(), lr=1e-4, weight_decay=1e-2)
    _step_and_check(opt, "flow step k0 ch8")
    assert all(torch.equal(_bits(named[k]), v) for k, v in idle.items())
    assert len(opt.state) == len(named) - len(idle)

    torch.manual_seed(0)
    np.random.seed(0)
    D, side, S = 16, 16, 3
    conv_inn, cond_nets = CWFA.build_networks(D, side, S, internal_chans=8, cond_chans=4, with_lrnn=True, device="cuda")
    gen = torch.Generator().manual_seed(23)
    gt = torch.randn(1, D, side, side, generator=gen).cuda()
    views = torch.randn(1, 29, side, side, generator=gen).cuda()
    means = [(0.1 * torch.randn(1, D // 2 ** (n + 1), side, side, generator=gen)).cuda() for n in range(S - 1)]
    rates = dict(lr=1e-4, lr_first_step=3e-4, lr_cond=2e-5)
    opts = training.make_optimizers(conv_inn, cond_nets, weight_decay=0.0, **rates)
    mods = list(conv_inn) + list(cond_nets)
    start = {p: p.detach().clone() for m in mods for p in m.parameters()}
    res = training.train_iteration(conv_inn, cond_nets, gt, views, means, optimizers=opts, use_mean_branch=False)   # (the LRNN's mean branch is built for 512 x 512)
    assert all(np.isfinite(float(v)) for v in res["losses"])
    flat = [(o, n) for n, e in enumerate(opts) for o in (e if isinstance(e, tuple) else (e,))]
    assert len(flat) == 2 * (S - 1) + 1
    # the reference's ResidualBlocks share ONE PReLU slope (a default-argument instance, networks.py:200): it belongs to the condition
    # net of every flow step and takes one step of lr in each of their optimisers
    owners = {}
    for o, _ in flat:
        for p in o.param_groups[0]["params"]:
            owners[p] = owners.get(p, 0) + 1
    assert sorted(set(owners.values())) == [1, S - 1] and sum(1 for v in owners.values() if v > 1) == 1
    moved = 0
    for o, n in flat:
        (grp,) = o.param_groups
        lr = torch.tensor(grp["lr"], dtype=torch.float32, device="cuda")
        assert float(lr) == float(np.float32(rates["lr_first_step"] if n == S - 1 else rates["lr"] if o is opts[n][0] else rates["lr_cond"]))
        for p in grp["params"]:
            if "exp_avg" not in o.state.get(p, {}):
                assert torch.equal(_bits(p), _bits(start[p]))
                continue
            m = o.state[p]["exp_avg"]
            if owners[p] > 1:                           # k steps of exactly lr each, every one rounded once
                k = owners[p]
                assert float((p.detach() - start[p]).abs().max()) <= k * float(lr) + k * 2.0 ** -24 * float(start[p].abs().max() + k * lr)
                continue
            want = start[p] - lr * torch.sign(m)
            ok = (p.detach() == want) | ((m == 0) & (p.detach() == start[p]))
            if not bool(ok.all()):
                i = int((~ok).reshape(-1).nonzero()[0])
                vals = [float(t.detach().reshape(-1)[i]) for t in (start[p], p, m)]
                raise AssertionError(f"step {n}: {int((~ok).sum())} elements of a {tuple(p.shape)} parameter did not move by lr = {float(lr)!r}: "
                                     f"element {i} went {vals[0]!r} -> {vals[1]!r} with exp_avg {vals[2]!r}")
            moved += int((m != 0).sum())
    assert moved > 0.9 * sum(m.numel() for o, _ in flat for s in o.state.values() for m in s.values())
