#!/usr/bin/env python3
"""Time the benchmark's inverse pass (512 x 512 x 96, 4-scale CAT + LRNN, B = 1 -- bench.py's workload) in the split_bf16, bf16
and fp16 precision modes with HIP events: warm-up passes, then the median of the timed passes.  Prints one JSON line with
volumes/s per mode.
    python tools/amp_time.py [--steps 10] [--warmup 3] [--modes split_bf16,bf16,fp16]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cwfa_amd import CWFA, ops   # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="split_bf16,bf16,fp16")
    a = ap.parse_args()
    torch.manual_seed(0)
    np.random.seed(0)
    D, side, S = 96, 512, 5
    conv_inn, cond_nets = CWFA.build_networks(D, side, S, with_lrnn=True, device="cuda")
    g = torch.Generator().manual_seed(1)
    cond_input = torch.randn(1, 29, side, side, generator=g).cuda()
    mean_cache = [(0.1 * torch.randn(1, D // 2 ** (n + 1), side, side, generator=g)).cuda() for n in range(S - 1)]
    out = {"metric": "inverse_pass_throughput", "unit": "volumes/s", "workload": f"{side}x{side}x{D}, CAT x4 + LRNN, B=1",
           "steps": a.steps, "warmup": a.warmup, "value": {}, "ms_median": {}}
    for mode in a.modes.split(","):
        ops.set_precision(mode)
        with torch.no_grad():
            for _ in range(a.warmup):
                CWFA.inverse_pass(conv_inn, cond_nets, cond_input, mean_cache)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                CWFA.inverse_pass(conv_inn, cond_nets, cond_input, mean_cache)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        out["ms_median"][mode] = round(med, 3)
        out["value"][mode] = round(1000.0 / med, 2)
    ops.set_precision("fp32")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
