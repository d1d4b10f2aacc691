#!/usr/bin/env python3
"""Time the sample-axis posterior sampler on the MI355X and write profiles/posterior_sampler_time.json:

  * per kernel, at 512 x 512 with the detail-channel counts of the five halvings of a 96-plane volume (48, 24, 12, 6, 3), a CAT step's
    five coefficient stages (channel, row, channel, column, channel gathers, composed tables) and N = 32 samples, each with its own
    low: one ``ops.chain_inv_samples`` launch against 32 x (``sample_z_truncated`` + ``ops.chain_inv``), and the same launch with one
    low shared by all samples and with ``return_z``;
  * the benchmark's pyramid (96 x 512 x 512, LRNN, split-bf16 arithmetic): ``posterior_samples(32)`` with ``seed`` and without, and
    ``posterior_roi_means`` for 256 samples and 13 ROIs (one frame).

Protocol of tools/posterior_time.py: every form warmed up; HIP events around windows of calls; the compared forms alternate inside one
process; median (min, max) over the windows; the box's identity in the record.  Bytes are algorithmic: per sample 3 C planes (low in,
the pair out), plus the ten coefficient rows once.      python tools/posterior_sampler_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402


def per_kernel(quick):
    import torch
    from cwfa_amd import CWFA, ops
    H = W = 128 if quick else 512
    N = 4 if quick else 32
    g = torch.Generator().manual_seed(3)
    res = {}
    for C_ in (48, 24, 12, 6, 3):
        axes = (1, 2, 1, 3, 1)
        perms = [torch.randperm({1: C_, 2: H, 3: W}[ax], generator=g).cuda() for ax in axes]
        st = [ops.stage(0.3 * torch.randn(1, C_, H, W, device="cuda"), torch.randn(1, C_, H, W, device="cuda"), perm=p, axis=ax)
              for p, ax in zip(perms, axes)]
        lows = torch.randn(N, 1, C_, H, W, device="cuda")
        tabs = ops.chain_tables(list(zip(perms, axes)), None, C_, H, W, lows.device)

        def per_sample():
            return [ops.chain_inv(CWFA.sample_z_truncated(lows[i], device="cuda", temperature=1.0), lows[i], st, tables=tabs) for i in range(N)]

        def per_sample_seeded_draw():
            return [ops.chain_inv(CWFA.sample_z_truncated(lows[i], device="cuda", temperature=1.0, seed=5, sample_offset=i), lows[i], st, tables=tabs)
                    for i in range(N)]

        fns = {"samples_launch": lambda: ops.chain_inv_samples(lows, st, N, 1.0, 5, tables=tabs),
               "per_sample_torch_draw": per_sample,
               "samples_launch_shared_low": lambda: ops.chain_inv_samples(lows[0], st, N, 1.0, 5, tables=tabs),
               "samples_launch_return_z": lambda: ops.chain_inv_samples(lows, st, N, 1.0, 5, tables=tabs, return_z=True),
               "per_sample_one_launch_draw": per_sample_seeded_draw}
        plane = 4 * C_ * H * W
        planes = {"samples_launch": 3 * N + 10, "samples_launch_shared_low": 2 * N + 11, "samples_launch_return_z": 4 * N + 10,
                  "per_sample_torch_draw": None, "per_sample_one_launch_draw": None}
        ms = windows(fns, 3 if quick else 9, 2 if quick else 5, 2)
        res[f"C{C_}"] = {k: dict(summary(v, planes[k] * plane if planes[k] else None), samples=N, ms_per_sample=round(summary(v)["ms"] / N, 5))
                         for k, v in ms.items()}
        res[f"C{C_}"]["speedup_vs_per_sample"] = round(res[f"C{C_}"]["per_sample_torch_draw"]["ms"] / res[f"C{C_}"]["samples_launch"]["ms"], 2)
        assert torch.equal(fns["samples_launch"](), fns["samples_launch"]())
        del lows, st
        torch.cuda.empty_cache()
    res["sizes"] = {"H": H, "W": W, "samples": N, "stages": 5}
    return res


def pyramid(quick):
    import numpy as np
    import torch
    from cwfa_amd import CWFA, ops
    torch.manual_seed(0)
    side, D, S = (128, 32, 3) if quick else (512, 96, 5)
    ops.set_precision("split_bf16")
    try:
        conv_inn, cond_nets = CWFA.build_networks(D, side, S, with_lrnn=not quick, device="cuda")
        g = torch.Generator().manual_seed(1)
        cond_input = torch.randn(1, 29, side, side, generator=g).cuda()
        mean_cache = [(0.1 * torch.randn(1, D // 2 ** (n + 1), side, side, generator=g)).cuda() for n in range(S - 1)]
        low = torch.randn(1, D // 2 ** (S - 1), side, side, generator=g).cuda() if quick else None
        N, NR = (4, 8) if quick else (32, 256)
        rs = np.random.RandomState(2)
        coords = [(int(rs.randint(8, side - 8)), int(rs.randint(8, side - 8)), int(rs.randint(-10, 10))) for _ in range(13)]
        boxes = CWFA.roi_boxes(coords, (1, D, side, side), 4, 2)
        args = (conv_inn, cond_nets, cond_input, mean_cache)
        fns = {f"posterior_samples_{N}_seeded": lambda: CWFA.posterior_samples(*args, N, low=low, temperature=1.0, seed=7),
               f"posterior_samples_{N}_unseeded": lambda: CWFA.posterior_samples(*args, N, low=low, temperature=1.0)}
        ms = windows(fns, 3 if quick else 7, 1 if quick else 3, 2)
        res = {k: summary(v) for k, v in ms.items()}
        a, b = res[f"posterior_samples_{N}_seeded"], res[f"posterior_samples_{N}_unseeded"]
        res["ms_per_sample_seeded"] = round(a["ms"] / N, 4)
        res["ms_per_sample_unseeded"] = round(b["ms"] / N, 4)
        res["seeded_faster_beyond_spread"] = bool(a["ms_max"] < b["ms_min"])
        res["speedup"] = round(b["ms"] / a["ms"], 2)
        roi = windows({"roi": lambda: CWFA.posterior_roi_means(*args, boxes, NR, low=low, temperature=1.0, seed=7, chunk=16)},
                      3 if quick else 5, 1, 1)
        res[f"posterior_roi_means_{NR}_samples_13_rois"] = dict(summary(roi["roi"]), note="ms per frame: networks once, 16 samples per chunk")
        res["config"] = {"depths": D, "side": side, "flow_steps": S - 1, "lrnn": not quick, "precision": "split_bf16", "batch": 1, "samples": N,
                         "note": "both forms run every network once per call (train-mode LRNN included); they differ in the per-sample work"}
        return res
    finally:
        ops.set_precision("fp32")


def main():
    import torch
    assert torch.cuda.is_available(), "posterior_sampler_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "sample-axis posterior sampler: one launch per step for N samples, latents drawn in the kernel",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, compared forms alternating in one process",
           "box": device_record(), "per_kernel": per_kernel(quick), "pyramid": pyramid(quick)}
    out = os.path.join(ROOT, "profiles", "posterior_sampler_time_quick.json" if quick else "posterior_sampler_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["pyramid"]))
    print(json.dumps({k: {n: (v["ms"], v.get("GBps")) for n, v in r.items() if isinstance(v, dict)} for k, r in rec["per_kernel"].items() if k != "sizes"}))


if __name__ == "__main__":
    main()
