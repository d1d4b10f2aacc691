#!/usr/bin/env python3
"""Time the weighted-MSE loss `wL2` forward plus gradient with HIP events at 96 x 512 x 512 (the finest flow step's volume) and at
6 x 512 x 512 (the LRNN step's), in one process and alternating:
  fused:  ops.global_extrema + ops.wmse_loss -- the two launches (three kernels plus the extrema finish) of DESIGN.md section 15;
  torch:  the reference's expression written with torch operators on the same tensors plus `.backward()` into the prediction, which
          is what the drop-in path ran before the fused pass existed.
Bytes are algorithmic for the fused form: 20 B per element (both tensors read by the extrema pass and again by the loss pass, the map
written once), reported against the 8000 GB/s DESIGN.md uses.  Writes one JSON file.
    python tools/loss_time.py [--repeats 30] [--steps 50] [--out profiles/loss_time.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cwfa_amd import ops   # noqa: E402

PEAK_GBPS = 8000.0


def torch_expression(output, target, ths_perc=0.05):
    so, st = output - output.min(), target - target.min()
    mo, mt = (so > so.max() * ths_perc).float(), (st > st.max() * ths_perc).float()
    return ((output - target) ** 2 * mo * mt).mean()


def event_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(fns, repeats, steps, warmup):
    """The callables in turn, `repeats` rounds of `steps` back-to-back calls each: {name: [ms per call, ...]}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            ms[k].append(event_ms(f, steps))
    return ms


def workload(shape, a):
    gen = torch.Generator(device="cuda").manual_seed(2323)
    gt = torch.clamp(0.7 * torch.randn(shape, generator=gen, device="cuda") + 0.2, min=0)
    pred = torch.clamp(gt + 0.15 * torch.randn(shape, generator=gen, device="cuda"), min=-0.1)
    n = gt.numel()
    leaf = pred.clone().requires_grad_()

    def fused():
        return ops.wmse_loss(gt, pred, gscale=1.0 / n, extrema=ops.global_extrema(gt, pred))

    def torch_form():
        leaf.grad = None
        torch_expression(gt, leaf).backward()
        return leaf.grad

    # the two forms compute the same thing on these tensors (the sign: the map is d / d gt)
    out, gmap = fused()
    want = torch_form()
    loss_t = float(torch_expression(gt, pred))
    agree = {"loss_fused": float(out[0]) / n, "loss_torch_fp32": loss_t, "in_mask_share": float(out[1]) / n,
             "max_abs_gradient_difference": float((gmap + want).abs().max()), "max_abs_gradient": float(want.abs().max())}
    ms = alternate({"fused": fused, "torch": torch_form}, a.repeats, a.steps, a.warmup)
    nbytes = 20 * n
    res = {"shape": list(shape), "elements": n, "bytes_fused_algorithmic": nbytes, "agreement": agree}
    for k, v in ms.items():
        med = statistics.median(v)
        res[k] = {"ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    f = res["fused"]
    f["GBps"] = round(nbytes / f["ms"] / 1e6, 1)
    f["fraction_of_8TBps"] = round(nbytes / f["ms"] / 1e6 / PEAK_GBPS, 3)
    res["speedup_vs_torch"] = round(res["torch"]["ms"] / f["ms"], 2)
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=30, help="timed rounds per form")
    ap.add_argument("--steps", type=int, default=50, help="back-to-back calls inside one timed window")
    ap.add_argument("--warmup", type=int, default=5, help="untimed rounds of both forms first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_time.py measures on the GPU; none is visible")
    out = {"workload": "wL2 loss forward + gradient map: extrema pass + loss pass (fused) vs the reference's torch expression + backward",
           "repeats": a.repeats, "steps_per_window": a.steps, "warmup_rounds": a.warmup,
           "note": "ms per call = median (min, max) over the windows of HIP-event time / steps, the two forms alternating in one process; "
                   "bytes algorithmic for the fused form, 20 B per element; fraction against 8000 GB/s"}
    out["flow_step_96x512x512"] = workload((1, 96, 512, 512), a)
    out["lrnn_step_6x512x512"] = workload((1, 6, 512, 512), a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
