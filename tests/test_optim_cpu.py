"""CPU: everything of the fused Lion optimiser that needs no GPU -- the C boundary of cwfa_lion_step_f32 and its argument checks,
the optimiser's constructor / param groups / state dict, the `lion_pytorch` drop-in of install(lion=True), make_optimizers, and the
float64 restatement tests/optim_ref.py against a plain torch-CPU fp32 evaluation of the same four lines."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import optim_ref
from cwfa_amd import _lib
from cwfa_amd.optim import Lion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from cwfa_amd import build
    build.build_all()
    return _lib.lib()


def test_entry_point_is_declared_bound_and_exported(L):
    src = open(os.path.join(ROOT, "include", "cwfa_hip.h")).read()
    assert re.search(r"\bint\s+cwfa_lion_step_f32\s*\(", src)
    assert int(re.search(r"#define\s+CWFA_LION_MAX_TENSORS\s+(\d+)", src).group(1)) == _lib.LION_MAX_TENSORS
    assert int(re.search(r"#define\s+CWFA_LION_BLOCK_ELEMS\s+(\d+)", src).group(1)) == _lib.LION_BLOCK_ELEMS
    assert "cwfa_lion_step_f32" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "cwfa_lion_step_f32")
    assert L.cwfa_version() == 100
    # the table and the per-tensor first-block list must fit the 4 KiB kernel-argument segment with the scalars
    assert ctypes.sizeof(_lib.LionTable) + 4 * _lib.LION_MAX_TENSORS + 64 <= 3584
    from cwfa_amd import build
    assert "optim_ops.hip" in build.SOURCES


def test_argument_validation_without_gpu(L):
    def call(tab):
        return L.cwfa_lion_step_f32(ctypes.byref(tab), 1e-4, 0.9, 0.99, 0.0, None, None, None)
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    tab = _lib.LionTable()
    assert call(tab) == 0                                               # n = 0: nothing to do, no launch
    tab.n = 3                                                           # only empty tensors (null pointers allowed): no launch
    assert call(tab) == 0
    tab.n = _lib.LION_MAX_TENSORS + 1
    assert call(tab) == -1 and b"not in 0" in L.cwfa_last_error()
    tab.n = -1
    assert call(tab) == -1 and b"not in 0" in L.cwfa_last_error()
    tab.n = 2
    tab.t[1].p = tab.t[1].g = tab.t[1].m = ptr
    tab.t[1].numel = -4
    assert call(tab) == -1 and b"negative" in L.cwfa_last_error()
    tab.t[1].numel = 1 << 31
    assert call(tab) == -2 and b"2^31" in L.cwfa_last_error()
    tab.t[1].numel = 4
    for field in ("p", "g", "m"):
        setattr(tab.t[1], field, None)
        assert call(tab) == -1 and b"tensor 1 has a null pointer" in L.cwfa_last_error(), field
        setattr(tab.t[1], field, ptr)
    tab.t[1].g = ptr + 2
    assert call(tab) == -3 and b"aligned" in L.cwfa_last_error()
    assert L.cwfa_lion_step_f32(None, 1e-4, 0.9, 0.99, 0.0, None, None, None) == -1


def test_constructor_validation():
    w = torch.nn.Parameter(torch.zeros(3))
    for bad in (0.0, -1e-3):
        with pytest.raises(ValueError, match="learning rate"):
            Lion([w], lr=bad)
    for bad in ((1.0, 0.9), (0.9, 1.0), (-0.1, 0.9), (0.9,)):
        with pytest.raises(ValueError, match="beta"):
            Lion([w], betas=bad)
    with pytest.raises(ValueError, match="learning rate"):
        Lion([{"params": [w], "lr": 0.0}], lr=1e-4)
    with pytest.raises(ValueError, match="beta"):
        Lion([{"params": [w], "betas": (0.9, 1.5)}])
    opt = Lion([w])
    assert opt.defaults == {"lr": 1e-4, "betas": (0.9, 0.99), "weight_decay": 0.0}
    assert Lion._step_supports_amp_scaling is True
    import inspect
    assert "grad_scaler" not in inspect.signature(opt.step).parameters


def test_param_groups_keep_their_own_rates():
    a, b, c = (torch.nn.Parameter(torch.zeros(n)) for n in (2, 3, 4))
    opt = Lion([{"params": iter([a]), "lr": 3e-4, "weight_decay": 1e-2}, {"params": [b], "betas": (0.5, 0.5)}, {"params": [c]}], lr=1e-5)
    g0, g1, g2 = opt.param_groups
    assert (g0["lr"], g0["weight_decay"], g0["betas"]) == (3e-4, 1e-2, (0.9, 0.99)) and g0["params"] == [a]
    assert (g1["lr"], g1["weight_decay"], g1["betas"]) == (1e-5, 0.0, (0.5, 0.5))
    assert (g2["lr"], g2["weight_decay"], g2["betas"]) == (1e-5, 0.0, (0.9, 0.99))


def test_state_dict_round_trip_and_lion_pytorch_layout():
    a, b = torch.nn.Parameter(torch.randn(2, 3)), torch.nn.Parameter(torch.randn(5))
    opt = Lion([{"params": [a], "lr": 3e-4, "weight_decay": 1e-2}, {"params": [b]}], lr=1e-5)
    assert opt.state_dict()["state"] == {}                              # created by the first step that sees a gradient
    opt.state[a]["exp_avg"] = torch.full_like(a, 0.25)                  # (what a step on the device leaves behind)
    sd = opt.state_dict()
    assert set(sd["state"]) == {0} and set(sd["state"][0]) == {"exp_avg"}
    a2, b2 = torch.nn.Parameter(torch.zeros(2, 3)), torch.nn.Parameter(torch.zeros(5))
    opt2 = Lion([{"params": [a2]}, {"params": [b2]}])
    opt2.load_state_dict(sd)
    assert torch.equal(opt2.state[a2]["exp_avg"], torch.full_like(a, 0.25)) and b2 not in opt2.state
    assert opt2.param_groups[0]["lr"] == 3e-4 and opt2.param_groups[0]["weight_decay"] == 1e-2 and opt2.param_groups[1]["lr"] == 1e-5
    sd2 = opt2.state_dict()
    assert sd2["param_groups"] == sd["param_groups"] and torch.equal(sd2["state"][0]["exp_avg"], sd["state"][0]["exp_avg"])
    # a state dict as lion_pytorch writes it (CWFA.py serialize_INN_step: optimizer.state_dict()): exp_avg per parameter index,
    # groups with lr / betas / weight_decay; float64 moments are cast to the parameter's dtype by the base class
    hand = {"state": {0: {"exp_avg": torch.arange(6.0, dtype=torch.float64).reshape(2, 3)}, 1: {"exp_avg": torch.ones(5)}},
            "param_groups": [{"lr": 2e-4, "betas": (0.95, 0.98), "weight_decay": 0.01, "params": [0]},
                             {"lr": 1e-4, "betas": (0.9, 0.99), "weight_decay": 0.0, "params": [1]}]}
    opt3 = Lion([{"params": [a2]}, {"params": [b2]}])
    opt3.load_state_dict(hand)
    assert opt3.state[a2]["exp_avg"].dtype == torch.float32 and torch.equal(opt3.state[a2]["exp_avg"], torch.arange(6.0).reshape(2, 3))
    assert torch.equal(opt3.state[b2]["exp_avg"], torch.ones(5))
    assert opt3.param_groups[0]["betas"] == (0.95, 0.98) and opt3.param_groups[0]["weight_decay"] == 0.01


def test_install_lion_registers_the_drop_in_module():
    import cwfa_amd
    saved = dict(sys.modules)
    try:
        sys.modules.pop("lion_pytorch", None)
        cwfa_amd.install()
        assert "lion_pytorch" not in sys.modules                        # the default registers what it always registered
        cwfa_amd.install(lion=True)
        from lion_pytorch import Lion as Dropped
        assert Dropped is Lion
        import networks
        assert networks is cwfa_amd.networks
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)


def test_step_on_cpu_parameters_raises(L):
    from cwfa_amd import ops
    w = torch.nn.Parameter(torch.zeros(4))
    w.grad = torch.ones(4)
    opt = Lion([w])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(w.detach(), torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lion_step([w.detach()], [w.grad], [torch.zeros(4)], 1e-4, (0.9, 0.99), 0.0)
    x = torch.nn.Parameter(torch.zeros(4, 4).t())                       # not contiguous: refused before anything else
    x.grad = torch.ones(4, 4)
    with pytest.raises(RuntimeError, match="not contiguous"):
        Lion([x]).step()
    Lion([torch.nn.Parameter(torch.zeros(2))]).step()                   # no gradient anywhere: nothing to do, nothing raised


def test_make_optimizers_structure_and_rates():
    from cwfa_amd import CWFA, training
    torch.manual_seed(0)
    np.random.seed(0)
    conv_inn, cond_nets = CWFA.build_networks(16, 16, 3, internal_chans=8, cond_chans=4, with_lrnn=True, device="cpu")
    opts = training.make_optimizers(conv_inn, cond_nets, lr=1e-4, lr_first_step=3e-4, lr_cond=2e-5, weight_decay=1e-2)
    assert len(opts) == 3
    for n in (0, 1):
        flow, cond = opts[n]
        assert isinstance(flow, Lion) and isinstance(cond, Lion)
        (g,) = flow.param_groups
        assert g["lr"] == 1e-4 and g["weight_decay"] == 1e-2 and g["betas"] == (0.9, 0.99)
        assert [id(p) for p in g["params"]] == [id(p) for p in conv_inn[n].parameters()]
        (g,) = cond.param_groups
        assert g["lr"] == 2e-5 and g["weight_decay"] == 0.0
        assert [id(p) for p in g["params"]] == [id(p) for p in cond_nets[n].parameters()]
    assert isinstance(opts[2], Lion)
    (g,) = opts[2].param_groups
    assert g["lr"] == 3e-4 and g["weight_decay"] == 1e-2
    assert [id(p) for p in g["params"]] == [id(p) for p in cond_nets[2].parameters()]
    only = training.make_optimizers(conv_inn, cond_nets, 1e-4, 3e-4, 2e-5, 1e-2, steps=[1])
    assert only[0] is None and only[2] is None and isinstance(only[1], tuple)
    with pytest.raises(ValueError):
        training.make_optimizers(conv_inn, cond_nets, 1e-4, 3e-4, 2e-5, 1e-2, steps=[3])
    flows = training.make_optimizers(conv_inn, cond_nets[:2], 1e-4, 3e-4, 2e-5, 1e-2)
    assert len(flows) == 2 and all(isinstance(o, tuple) for o in flows)


def _torch_fp32_step(p, g, m, lr, betas, wd, scale=None):
    """The four lines with torch CPU operators in fp32, one rounding per operation, hyper-parameters as the kernel holds them."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)                  # noqa: E731
    lr_, b1, b2, wd_ = f(lr), f(betas[0]), f(betas[1]), f(wd)
    gp = g if scale is None else g / f(scale)
    c = b1 * m + (f(1.0) - b1) * gp
    p1 = p * (f(1.0) - lr_ * wd_) - lr_ * torch.sign(c)
    m1 = b2 * m + (f(1.0) - b2) * gp
    return p1, m1


@pytest.mark.parametrize("lr,betas,wd,scale", [(1e-4, (0.9, 0.99), 0.0, None), (3e-4, (0.9, 0.99), 1e-2, None),
                                               (1e-3, (0.5, 0.5), 1e-2, 4.0), (1e-4, (0.95, 0.98), 0.1, 3.0)])
def test_reference_agrees_with_a_plain_fp32_evaluation(lr, betas, wd, scale):
    rng = np.random.default_rng(0)
    n = 1 << 18
    p, g, m = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    if scale is not None:
        g = g * np.float32(scale)
    ref = optim_ref.lion_step(p, g, m, lr, betas, wd, scale)
    assert ref["ambiguous"].mean() <= optim_ref.AMBIGUOUS_CAP
    p1, m1 = _torch_fp32_step(torch.from_numpy(p), torch.from_numpy(g), torch.from_numpy(m), lr, betas, wd, scale)
    optim_ref.check(p1.numpy(), m1.numpy(), ref, f"lr={lr} betas={betas} wd={wd} scale={scale}")
    # and the reference really is the update rule: signs and magnitudes on a hand-made case
    r = optim_ref.lion_step([1.0, -2.0, 0.5], [0.5, -0.5, 0.0], [0.0, 1.0, 0.0], 0.125, (0.5, 0.25), 0.5)
    assert np.array_equal(r["p"], np.array([1.0 * 0.9375 - 0.125, -2.0 * 0.9375 - 0.125, 0.5 * 0.9375]))
    assert np.array_equal(r["m"], np.array([0.375, 0.25 - 0.375, 0.0]))
    assert list(r["ambiguous"]) == [False, False, True]
