"""CPU: the weighted-MSE loss `wL2` away from the device -- the plain-torch restatement tests/loss_ref.py
against the fixtures g23_wmse* (the reference's own losses.weighted_mse_loss with torch autograd: tools/make_loss_golden.py), the
extrema exchange between ranks, the `losses` name of install(), and what the host code refuses without a GPU."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import loss_ref as R

CASES = ["odd_tail", "two_samples", "blocks_and_tail", "constant_pred", "ths_zero", "disjoint"]


@pytest.fixture(scope="module")
def table():
    return R.load()


def test_fixture_holds_every_case(table):
    assert sorted(table) == sorted(CASES)
    assert [table[n]["gt"].shape for n in CASES[:3]] == [(1, 3, 5, 7), (2, 6, 33, 37), (1, 6, 128, 130)]
    for n in CASES[:3]:
        c = table[n]
        assert 0.25 <= int(c["count32"]) / c["gt"].size <= 0.75 and c["ths_perc"] == 0.05 and float(c["ref32_err"]) > 0
    for n in ("constant_pred", "disjoint"):
        assert int(table[n]["count32"]) == 0 and float(table[n]["loss32"]) == 0 and not table[n]["grad32"].any()
    assert table["ths_zero"]["ths_perc"] == 0.0 and int(table["ths_zero"]["count32"]) > 0


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(table, name):
    """fp32: the loss and the gradient bit for bit, the count exactly; float64 on the same fp32 inputs: to rounding."""
    c = table[name]
    gt, pred = torch.from_numpy(c["gt"]), torch.from_numpy(c["pred"])
    loss, grad, count = R.loss_grad_count(gt, pred, c["ths_perc"])
    assert loss.dtype == torch.float32 and grad.dtype == torch.float32
    assert count == int(c["count32"]) == int(c["count64"])
    assert np.array_equal(loss.numpy(), c["loss32"]), (float(loss), float(c["loss32"]))
    assert np.array_equal(grad.numpy(), c["grad32"])
    # the other argument order: the same loss, the negated gradient for the prediction
    loss_r, grad_r, count_r = R.loss_grad_count(pred, gt, c["ths_perc"])
    assert count_r == count and np.array_equal(grad_r.numpy(), -c["grad32"])
    loss64, grad64, count64 = R.loss_grad_count(gt.double(), pred.double(), c["ths_perc"])
    assert count64 == count
    assert abs(float(loss64) - float(c["loss64"])) <= 1e-14 * abs(float(c["loss64"]))
    assert np.allclose(grad64.numpy(), c["grad64"], rtol=1e-14, atol=0)
    assert abs(float(loss) - float(c["loss64"])) == float(c["ref32_err"])
    if int(c["count32"]):                               # the stored fp32 gradient itself is inside the bound the kernel is held to
        R.check_grad(c["grad32"], c, what=name)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _extrema_row(a, b):
    row = torch.zeros(12)
    row[0], row[1], row[4], row[5] = a.min(), a.max(), b.min(), b.max()
    row[2], row[8] = 7.0, -3.0                            # slots the exchange must leave alone
    return row


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cwfa_amd import training
        c = R.load()["two_samples"]
        gt, pred = torch.from_numpy(c["gt"]), torch.from_numpy(c["pred"])
        ext = training.allreduce_extrema(_extrema_row(gt[rank:rank + 1], pred[rank:rank + 1]))
        q.put((rank, ext.tolist(), _extrema_row(gt[rank:rank + 1], pred[rank:rank + 1]).tolist()))
    finally:
        dist.destroy_process_group()


def test_allreduce_extrema_two_ranks_gloo(table):
    """Each rank holds one sample of `two_samples`: after the exchange both hold the extrema of the whole batch."""
    c = table["two_samples"]
    gt, pred = torch.from_numpy(c["gt"]), torch.from_numpy(c["pred"])
    want = _extrema_row(gt, pred).tolist()
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == [0, 1]
    local = {r[0]: r[2] for r in res}
    assert local[0] != local[1] and want not in (local[0], local[1]), "the shards must differ for the test to mean anything"
    for _, ext, _ in res:
        assert ext == want


def test_allreduce_extrema_is_a_no_op_without_a_group():
    from cwfa_amd import training
    row = _extrema_row(torch.tensor([1.0, -2.0]), torch.tensor([0.5, 4.0]))
    out = training.allreduce_extrema(row.clone())
    assert torch.equal(out, row)


def test_install_registers_losses_only_on_request():
    import cwfa_amd
    keep = {k: sys.modules.get(k) for k in ("losses", "FrEIA", "FrEIA.framework", "FrEIA.modules", "INN_utils", "networks", "unet")}
    try:
        sys.modules.pop("losses", None)
        cwfa_amd.install()
        assert "losses" not in sys.modules
        cwfa_amd.install(losses=True)
        import losses as Losses
        from cwfa_amd import losses as ours
        assert Losses is ours and Losses.weighted_mse_loss is ours.weighted_mse_loss
        assert ours.__all__ == ["weighted_mse_loss"] and "only what CWFA.py" in " ".join(ours.__doc__.split())
    finally:
        for k, v in keep.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_loss_refuses_what_it_cannot_run():
    """No CPU path, LL stays unbuilt, and the C entry validates its arguments before anything is launched (no GPU here)."""
    from cwfa_amd import _lib, build, losses, ops, training
    build.build_all()
    a = torch.zeros(1, 2, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wmse_loss(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.weighted_mse_loss(a, a)
    with pytest.raises(NotImplementedError, match="LL"):
        training.lrnn_step_backward(None, None, None, None, loss_func="LL")
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.cwfa_wmse_loss_f32(p, p, p, 0.05, 1.0, None, None, p, 16, None) == -1
    assert b"null out" in L.cwfa_last_error()
    assert L.cwfa_wmse_loss_f32(p, p, p, 0.05, 1.0, None, p, p, -1, None) == -1
    assert b"negative" in L.cwfa_last_error()
    assert L.cwfa_wmse_loss_f32(None, p, p, 0.05, 1.0, None, p, p, 16, None) == -1
    assert b"null pointer" in L.cwfa_last_error()
    assert L.cwfa_wmse_workspace_bytes(-1) == -1 and L.cwfa_wmse_workspace_bytes(0) == 0
    assert L.cwfa_wmse_workspace_bytes(1) == 16 and L.cwfa_wmse_workspace_bytes(5000) == 32
    assert L.cwfa_wmse_workspace_bytes(96 * 512 * 512) == 2048 * 16
