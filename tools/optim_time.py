#!/usr/bin/env python3
"""Time one optimiser step (cwfa_amd.optim.Lion: cwfa_lion_step_f32, one launch per 96 tensors) with HIP events over (a) the finest
flow step plus its condition net and (b) the LRNN, both from CWFA.build_networks() defaults with random gradients.  In the same
process and alternating with it: the same update written with torch's `_foreach_` operators in fp32 over the same tensors (the four
lines of the rule as lion_pytorch writes them, seven multi-tensor operators per group).  Bytes are algorithmic: 20 B per parameter
(p, g, m read; p, m written), reported against the 8000 GB/s DESIGN.md uses.  Launch counts come from torch.profiler's kernel events
of one step.  Writes one JSON file.
    python tools/optim_time.py [--repeats 30] [--steps 20] [--out profiles/optim_time.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cwfa_amd import CWFA, _lib   # noqa: E402
from cwfa_amd.optim import Lion   # noqa: E402

PEAK_GBPS = 8000.0
BETAS = (0.9, 0.99)


def foreach_step(groups):
    """lion_pytorch's update_fn over lists: p *= 1 - lr wd;  u = sign(b1 m + (1 - b1) g);  p -= lr u;  m = b2 m + (1 - b2) g."""
    b1, b2 = BETAS
    for ps, gs, ms, lr, wd in groups:
        torch._foreach_mul_(ps, 1.0 - lr * wd)
        u = torch._foreach_mul(ms, b1)
        torch._foreach_add_(u, gs, alpha=1.0 - b1)
        torch._foreach_sign_(u)
        torch._foreach_add_(ps, u, alpha=-lr)
        torch._foreach_mul_(ms, b2)
        torch._foreach_add_(ms, gs, alpha=1.0 - b2)


def event_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(fns, repeats, steps, warmup):
    """The callables in turn, `repeats` rounds of `steps` back-to-back steps each: {name: [ms per step, ...]}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            ms[k].append(event_ms(f, steps))
    return ms


def kernel_launches(fn):
    """Device kernels of one call, from torch.profiler; None where the profiler is not usable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as exc:                                # noqa: BLE001
        print(f"launch count not measured: {exc}", file=sys.stderr)
        return None


def workload(name, specs, a):
    """specs: [(module, lr, wd)] -- one Lion optimiser per entry (as training.make_optimizers builds them) and the foreach groups
    over the same parameters and gradients with a moment list of their own."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    opts, groups, n_params, n_tensors = [], [], 0, 0
    for mod, lr, wd in specs:
        ps = [p for p in mod.parameters() if p.requires_grad]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen, device="cuda")
        opts.append(Lion([{"params": ps, "lr": lr, "weight_decay": wd}], lr=lr, betas=BETAS))
        groups.append(([p.detach() for p in ps], [p.grad for p in ps], [torch.zeros_like(p) for p in ps], lr, wd))
        n_params += sum(p.numel() for p in ps)
        n_tensors += len(ps)

    def fused():
        for o in opts:
            o.step()

    def foreach():
        foreach_step(groups)

    ms = alternate({"fused": fused, "foreach": foreach}, a.repeats, a.steps, a.warmup)
    nbytes = 20 * n_params
    out = {"parameters": n_params, "tensors": n_tensors, "bytes": nbytes}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "GBps": round(nbytes / med / 1e6, 1),
                  "fraction_of_peak": round(nbytes / med / 1e6 / PEAK_GBPS, 3)}
    out["fused"]["launches"] = sum(-(-len(g[0]) // _lib.LION_MAX_TENSORS) for g in groups)
    out["fused"]["launches_profiled"] = kernel_launches(fused)
    out["foreach"]["launches_profiled"] = kernel_launches(foreach)
    spread = out["foreach"]["ms_max"] - out["foreach"]["ms_min"]
    out["foreach_spread_ms"] = round(spread, 4)
    out["fused_not_slower_than_foreach_by_more_than_its_spread"] = out["fused"]["ms"] <= out["foreach"]["ms"] + spread
    out["speedup_vs_foreach"] = round(out["foreach"]["ms"] / out["fused"]["ms"], 2)
    print(name, json.dumps(out))
    for mod, _, _ in specs:
        for p in mod.parameters():
            p.grad = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=30, help="timed rounds per form")
    ap.add_argument("--steps", type=int, default=20, help="back-to-back optimiser steps inside one timed window")
    ap.add_argument("--warmup", type=int, default=10, help="untimed rounds of both forms first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_time.py measures on the GPU; none is visible")
    torch.manual_seed(0)
    conv_inn, cond_nets = CWFA.build_networks()
    out = {"workload": "one Lion step, networks of CWFA.build_networks() defaults (96 x 512 x 512, 5 steps), random gradients",
           "repeats": a.repeats, "steps_per_window": a.steps, "warmup_rounds": a.warmup,
           "note": "ms per step = median (min, max) over the windows of HIP-event time / steps, the two forms alternating in one process; "
                   "bytes algorithmic, 20 B per parameter; fraction_of_peak against 8000 GB/s"}
    out["finest_flow_step_and_condition_net"] = workload("flow0+cond0", [(conv_inn[0], 1e-4, 1e-2), (cond_nets[0], 1e-4, 0.0)], a)
    out["lrnn"] = workload("lrnn", [(cond_nets[-1], 1e-4, 1e-2)], a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
