#!/usr/bin/env python3
"""Time the trace post-processing on the MI355X and write profiles/traces_time.json.

Float64 traces [N, T], T = 10 000, N = 200 and N = 4096, half window 300 (W = 601), percentile 8, gamma = 0.95, lam = 2 sigma, one GPU
process.  The traces are a seeded version of the test scene at recording length: a bleaching, drifting baseline times (1 + calcium)
plus noise.

  * ``trace_baseline`` in the LDS form and in the streaming form;
  * ``trace_noise``;
  * ``infer_spikes`` with ``lam_sigma`` (the noise level and the deconvolution) and ``ops.ar1_deconv`` alone;
  * the torch form of the baseline: ``unfold`` + ``sort`` of the edge-padded trace over TORCH_ROWS rows at a time (what fits in
    memory beside the sort's index tensor), timed on one such slab and, at N = 4096, NOT run over all rows: the record says how many
    rows were timed;
  * the CPU restatement's row loop of the deconvolution (tests/traces_ref.py) on CPU_ROWS rows: host time, per row.

Every device form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over
the windows.  The baseline kernels are not bound by the 16 bytes per element they move, so their records carry the count of LDS (or
memory) reads per output instead of a byte floor.
    python tools/traces_time.py [--quick]"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from posterior_time import device_record, summary, windows      # noqa: E402

TORCH_ROWS, CPU_ROWS = 64, 4


def traces(N, T, rng):
    """The scene of tests/traces_ref.py at recording length, made on the host and uploaded."""
    import numpy as np
    import torch
    t = np.arange(T, dtype=np.float64)
    c = (rng.random((N, T)) < 0.03) * (0.5 + rng.random((N, T)))
    for i in range(1, T):                                                         # the AR(1) response, in place, all rows at once
        c[:, i] += 0.9 * c[:, i - 1]
    base = (2 + 2 * rng.random((N, 1))) * (0.6 + 0.4 * np.exp(-t / (T / 2.4))) * (1 + 0.1 * np.sin(2 * np.pi * t / (T / 1.5) + 6 * rng.random((N, 1))))
    return torch.from_numpy(base * (1 + c) + 0.1 * rng.standard_normal((N, T))).cuda()


def torch_baseline(x, h, p):
    """The torch-operator form: every window materialised and sorted."""
    import torch
    T = x.shape[1]
    padded = torch.nn.functional.pad(x, (h, h), value=float("inf"))
    out = torch.empty_like(x)
    m = torch.minimum(torch.arange(T, device=x.device) + h, torch.tensor(T - 1, device=x.device)) - (torch.arange(T, device=x.device) - h).clamp_min(0)
    k = (p * m) // 100
    for r0 in range(0, x.shape[0], TORCH_ROWS):
        s = padded[r0:r0 + TORCH_ROWS].unfold(1, 2 * h + 1, 1).sort(dim=2).values
        out[r0:r0 + TORCH_ROWS] = s.gather(2, k[None, :, None].expand(s.shape[0], T, 1))[:, :, 0]
    return out


def measure(quick):
    import numpy as np
    import torch
    import traces_ref as R
    from cwfa_amd import CWFA, ops
    T, h, p, gamma = (2000, 60, 8, 0.95) if quick else (10000, 300, 8, 0.95)
    tile, most = ops.sliding_quantile_limits()
    rng = np.random.default_rng(9)
    res = {}
    for N in ((16, 128) if quick else (200, 4096)):
        x = traces(N, T, rng)
        lam = 2.0 * CWFA.trace_noise(x)
        big = N > 1000
        fast = {"baseline_lds": lambda: ops.sliding_quantile(x, h, p, form="lds"), "trace_noise": lambda: CWFA.trace_noise(x),
                "infer_spikes_lam_sigma": lambda: CWFA.infer_spikes(x, gamma, lam_sigma=2.0), "ar1_deconv": lambda: ops.ar1_deconv(x, gamma, lam)}
        ms = windows(fast, 3 if quick else 7, 1, 1)
        rows = min(N, TORCH_ROWS)
        slow = {"baseline_stream": lambda: ops.sliding_quantile(x, h, p, form="stream"),
                "torch_unfold_sort_slab": lambda: torch_baseline(x[:rows], h, p)}
        ms.update(windows(slow, 2 if big else 3, 1, 1))
        r = {k: summary(v) for k, v in ms.items()}
        M = min(T, tile + 2 * h)
        bits = max(1, math.ceil(math.log2(M)))
        groups = (2 * h + 1 + 14) // 8                                          # SQ_GROUPS(h) of csrc/trace_ops.hip
        r["baseline_lds"]["lds_reads_per_output"] = {"bisection_16_byte_of_8_ranks": groups * bits, "bisection_2_byte": 21 * bits,
                                                     "ranking_8_byte_same_address_per_wave": M * math.ceil(M / (4 * tile)),
                                                     "a_64_step_bisection_on_8_byte_keys_would_take": 64 * (2 * h + 1), "staged_samples": M, "rank_bits": bits}
        r["baseline_lds"]["outputs_per_second"] = round(N * T / r["baseline_lds"]["ms"] * 1e3)
        r["baseline_stream"]["memory_reads_per_output"] = 64 * (2 * h + 1)
        r["torch_unfold_sort_slab"]["rows_timed"] = rows
        r["torch_unfold_sort_slab"]["ms_per_row"] = round(r["torch_unfold_sort_slab"]["ms"] / rows, 4)
        r["torch_unfold_sort_slab"]["all_rows_ms_at_this_rate_not_measured"] = round(r["torch_unfold_sort_slab"]["ms"] / rows * N, 1)
        if big or quick:                                                          # the LDS form over its range of half windows
            sweep = (0, 10, 100) if quick else (0, 50, 1000, most)
            by_h = windows({f"h{hh}": (lambda hh=hh: ops.sliding_quantile(x, hh, p, form="lds")) for hh in sweep}, 3, 1, 1)
            r["baseline_lds_by_half_window"] = {k: dict(summary(v), staged_samples=min(T, tile + 2 * int(k[1:])),
                                                        ranking_passes=math.ceil(min(T, tile + 2 * int(k[1:])) / (4 * tile))) for k, v in by_h.items()}
        xs = x[:CPU_ROWS].cpu().numpy()
        ls = lam[:CPU_ROWS].cpu().numpy()
        t0 = time.perf_counter()
        want = R.ar1_deconv(xs, gamma, ls)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        r["cpu_restatement_deconv"] = {"rows_timed": CPU_ROWS, "host_ms_per_row": round(cpu_ms / CPU_ROWS, 2),
                                       "all_rows_ms_at_this_rate_not_measured": round(cpu_ms / CPU_ROWS * N, 1)}
        c, s, pools = ops.ar1_deconv(x, gamma, lam)
        base = ops.sliding_quantile(x, h, p, form="lds")
        tb = torch_baseline(x[:rows], h, p)
        r["checks"] = {"forms_agree": bool(torch.equal(base, ops.sliding_quantile(x, h, p, form="stream"))),
                       "torch_form_agrees_on_its_rows": bool(torch.equal(tb, base[:rows])),
                       "deconv_equals_restatement_on_its_rows": bool(np.array_equal(c[:CPU_ROWS].cpu().numpy(), want[0]) and np.array_equal(s[:CPU_ROWS].cpu().numpy(), want[1])),
                       "pools_min_median_max": [int(pools.min()), float(pools.double().median()), int(pools.max())],
                       "nonzero_spikes_per_row_median": float((s > 0).sum(1).double().median())}
        r["config"] = {"rows": N, "deconv_workspace_bytes": (20 * N * T + 7) // 8 * 8}
        res[f"N{N}"] = r
        del x, c, s, base, tb
    res["config"] = {"T": T, "half_window": h, "percentile": p, "gamma": gamma, "lam": "2 sigma", "tile": tile, "max_half_lds": most,
                     "torch_rows_per_slab": TORCH_ROWS}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "traces_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "trace post-processing: sliding-quantile baseline (both forms), noise level, AR(1) deconvolution, and the torch / CPU forms",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "traces": measure(quick)}
    out = os.path.join(ROOT, "profiles", "traces_time_quick.json" if quick else "traces_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["traces"]))


if __name__ == "__main__":
    main()
