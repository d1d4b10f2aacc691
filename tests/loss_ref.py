"""CPU restatement of the weighted-MSE loss `wL2`, test infrastructure beside eval_ref.py / optim_ref.py: the
loss with plain torch operators in the dtype of its inputs (so torch.autograd differentiates it), the masks and the in-mask count,
and the bounds the GPU tests hold the kernel to.

    m_v  = (v - min v) > (max v - min v) * ths_perc              for v = output, target
    loss = mean((output - target)^2 * m_output * m_target)       (the mean over ALL elements)
"""
import numpy as np
import torch

GRAD_RTOL = 4.0 * 2.0 ** -24      # the map: three fp32 roundings (the difference, the scale 2 gscale, their product) and one spare


def masks(output, target, ths_perc=0.05):
    """The two boolean gates, in the arithmetic of the inputs' dtype."""
    so, st = output - output.min(), target - target.min()
    return so > so.max() * ths_perc, st > st.max() * ths_perc


def weighted_mse(output, target, ths_perc=0.05):
    mo, mt = masks(output.detach(), target.detach(), ths_perc)
    return ((output - target) ** 2 * (mo & mt).to(output.dtype)).mean()


def loss_grad_count(output, target, ths_perc=0.05):
    """(loss, d loss / d output, number of elements inside both masks) by torch.autograd, single-threaded so that the order of the
    fp32 mean does not depend on the machine's thread count.  The gradient for ``target`` is the negative of the one returned."""
    keep = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.enable_grad():
            o = output.detach().clone().requires_grad_()
            loss = weighted_mse(o, target.detach(), ths_perc)
            loss.backward()
        mo, mt = masks(output, target, ths_perc)
        return loss.detach(), o.grad, int((mo & mt).sum())
    finally:
        torch.set_num_threads(keep)


def load():
    """The cases of tests/golden/g23_wmse*.npz as one table {case: {gt, pred, ths_perc, loss32, grad32, count32, loss64, grad64, count64,
    ref32_err}} (tools/make_loss_golden.py; the largest case is spread over two files of its own)."""
    from conftest import load_golden
    fx, names = {}, []
    for f in ("g23_wmse", "g23_wmse_large", "g23_wmse_large_f64"):
        part = load_golden(f)
        names += [str(n) for n in part.pop("cases", [])]
        fx.update(part)
    return {n: case(fx, n) for n in names}


def case(fx, name):
    """One case of the loaded arrays as a dict (arrays as stored; ths_perc a python float)."""
    c = {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "/")}
    c["ths_perc"] = float(c["ths_perc"])
    return c


def check_grad(got, c, sign=1.0, what=""):
    """``got`` (fp32) against the stored gradients of d loss / d output times ``sign``: exactly zero where the stored fp32 gradient is
    zero, within GRAD_RTOL relative of the float64 gradient elsewhere.  Prints the worst ratio before asserting."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    g32, g64 = c["grad32"].reshape(-1), sign * c["grad64"].reshape(-1)
    zero = g32 == 0
    assert np.array_equal(zero, c["grad64"].reshape(-1) == 0), f"{what}: the fixture's fp32 and float64 gradients vanish in different places"
    assert not np.any(got[zero]), f"{what}: {int(np.count_nonzero(got[zero]))} non-zero gradients where the reference's are zero"
    worst = float(np.max(np.abs(got[~zero] - g64[~zero]) / np.abs(g64[~zero]), initial=0.0))
    print(f"{what}: worst |g - g64| / |g64| = {worst:.3e} (bound {GRAD_RTOL:.3e}), {int((~zero).sum())} of {zero.size} inside the masks")
    assert worst <= GRAD_RTOL, f"{what}: gradient off by {worst:.3e} relative"
