"""Write the loss fixtures tests/golden/g23_wmse.npz (and, to stay under the size limit for committed files, the largest case in two
files of its own: g23_wmse_large.npz, and g23_wmse_large_f64.npz with its float64 gradient; tests/loss_ref.py's load() reads the three
as one table): seeded inputs, ths_perc and the outputs of the REFERENCE's own losses.weighted_mse_loss with torch
autograd on the CPU (imported by oracle.make_golden's recipe) -- the fp32 loss, its fp32 gradient with respect to the first argument
and the in-mask count, and the same three from a float64 run on the same fp32 inputs.  Inputs, arguments and outputs only.  Run from
the repository root:  python tools/make_loss_golden.py

Per case `name`: name/gt, name/pred (the call is weighted_mse_loss(gt, pred, ths_perc), the argument order of CWFA.py:942,955),
name/ths_perc, name/loss32, name/grad32, name/count32, name/loss64, name/grad64, name/count64, and name/ref32_err = |loss32 - loss64|,
the error of the reference's own fp32 result, which the GPU test takes its bound from.

The generator asserts the conditions that keep the discrete gate from hiding an error.  Main cases: the in-mask share lies between
25 % and 75 %; the fp32 and float64 masks are equal; no element is within 64 ulps of its threshold.  Edge cases (a constant
prediction, ths_perc = 0, masks that do not intersect): the fp32 and float64 masks are equal and the result is what the case is for."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.make_golden import dump, import_reference  # noqa: E402

import loss_ref as R  # noqa: E402

MAIN = {"odd_tail": (1, 3, 5, 7), "two_samples": (2, 6, 33, 37), "blocks_and_tail": (1, 6, 128, 130)}
LARGE = ("blocks_and_tail",)


def npy(t):
    return t.detach().cpu().numpy()


def run(fn, gt, pred, ths):
    """The reference's function with autograd: (loss, d loss / d gt, in-mask count), in the dtype of gt / pred."""
    import torch
    with torch.enable_grad():
        o = gt.clone().requires_grad_()
        loss = fn(o, pred, ths)
        loss.backward()
    mo, mt = R.masks(gt, pred, ths)
    return loss.detach(), o.grad, int((mo & mt).sum())


def record(arrs, name, fn, gt, pred, ths, main):
    import torch
    l32, g32, c32 = run(fn, gt, pred, ths)
    l64, g64, c64 = run(fn, gt.double(), pred.double(), ths)
    m32, m64 = R.masks(gt, pred, ths), R.masks(gt.double(), pred.double(), ths)
    assert all(torch.equal(a, b) for a, b in zip(m32, m64)), f"{name}: the fp32 and float64 masks differ"
    assert c32 == c64 and c32 == int(np.count_nonzero(npy(g32))) == int(np.count_nonzero(npy(g64))), (name, c32, c64)
    if main:
        share = c32 / gt.numel()
        assert 0.25 <= share <= 0.75, f"{name}: in-mask share {share:.3f}"
        near = 0.0
        for v in (gt, pred):
            s = v - v.min()
            thr = s.max() * ths
            gap = ((s - thr).abs() / np.spacing(np.float32(thr))).min()
            assert float(gap) > 64, f"{name}: an element lies {float(gap):.1f} ulps from its threshold"
            near = max(near, 1.0 / float(gap))
        print(f"{name}: in-mask share {share:.3f}, nearest element {1 / near:.0f} ulps from its threshold")
    p = name + "/"
    arrs[p + "gt"], arrs[p + "pred"], arrs[p + "ths_perc"] = npy(gt), npy(pred), np.float64(ths)
    arrs[p + "loss32"], arrs[p + "grad32"], arrs[p + "count32"] = npy(l32), npy(g32), np.int64(c32)
    arrs[p + "loss64"], arrs[p + "grad64"], arrs[p + "count64"] = npy(l64), npy(g64), np.int64(c64)
    arrs[p + "ref32_err"] = np.float64(abs(float(l32.double()) - float(l64)))
    return l32, g32, c32


def main():
    import torch
    import_reference()
    import losses as RL                                  # the reference's losses.py (import_reference put it on the path)
    torch.set_num_threads(1)                             # the order of the fp32 mean must not depend on this machine's thread count
    fn = RL.weighted_mse_loss
    g = torch.Generator().manual_seed(2323)

    def pair(shape):
        gt = torch.clamp(0.7 * torch.randn(shape, generator=g) + 0.2, min=0)
        pred = torch.clamp(gt + 0.15 * torch.randn(shape, generator=g), min=-0.1)
        return gt, pred

    small, large = {}, {}
    for name, shape in MAIN.items():
        gt, pred = pair(shape)
        record(large if name in LARGE else small, name, fn, gt, pred, 0.05, True)
    # a constant prediction: range 0, so nothing is greater than the threshold 0 -- empty mask, loss 0, gradient all zero
    gt, _ = pair((1, 2, 5, 7))
    l, gr, c = record(small, "constant_pred", fn, gt, torch.full_like(gt, 0.3), 0.05, False)
    assert float(l) == 0 and c == 0 and not npy(gr).any()
    # ths_perc = 0: everything but the minima is inside
    gt, pred = pair((1, 2, 5, 7))
    l, gr, c = record(small, "ths_zero", fn, gt, pred, 0.0, False)
    assert 0 < c < gt.numel() and float(l) > 0
    # masks that do not intersect: each volume bright where the other is dark
    gt, pred = pair((1, 2, 5, 7))
    gt[:, 1], pred[:, 0] = 0.0, 0.0
    gt[:, 0] += 1.0
    pred[:, 1] += 1.0
    mo, mt = R.masks(gt, pred, 0.05)
    assert int(mo.sum()) > 0 and int(mt.sum()) > 0
    l, gr, c = record(small, "disjoint", fn, gt, pred, 0.05, False)
    assert float(l) == 0 and c == 0 and not npy(gr).any()
    for arrs in (small, large):
        arrs["cases"] = np.array(sorted({k.split("/")[0] for k in arrs}))
    dump("g23_wmse", **small)
    dump("g23_wmse_large_f64", **{k: large.pop(k) for k in [k for k in large if k.endswith("/grad64")]})
    dump("g23_wmse_large", **large)


if __name__ == "__main__":
    main()
