#!/usr/bin/env python3
"""Time the evaluation pass (cwfa_amd.CWFA.evaluate_step and its kernels) with HIP events at 512 x 512 x 96 and over the five
pyramid levels of one volume.  In the same process and alternating with it: (a) the same evaluation written with torch-ROCm
operators on the device (the float restatement of tests/eval_ref.py in fp32 on HIP tensors, projections kept on the device) and
(b) cwfa_sample_stats_f32 on the same tensor, the project's plain-reduction yardstick.  Also corr_coeff_3D for T = 32, N = 200.
Bytes are algorithmic (from the shapes).  Writes one JSON file; with --kernel-stats it starts ONE child of its own under
`rocprofv3 --kernel-trace --stats` and keeps that run's kernel table.
    python tools/eval_time.py [--repeats 9] [--out profiles/eval_time.json] [--kernel-stats profiles/eval_kernel_stats.csv]"""
import argparse
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cwfa_amd import CWFA, ops   # noqa: E402

STEP, MEAN, STD = 0, 0.31, 1.7


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, repeats, warmup=2):
    """Run the callables in turn, `repeats` rounds: {name: (median, min, max) ms}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            ms[k].append(event_ms(f))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def torch_projection(vol):
    """volume_2_projections' default call with torch operators, on the device."""
    v = vol.abs().permute(0, 2, 3, 1).unsqueeze(1)
    x, y, z = torch.amax(v, 2), torch.amax(v, 3), torch.amax(v, 4)
    B, _, H, W, D = v.shape
    s = 2 * D
    out = z.min() * torch.ones(B, 1, H + s + 2, W + s + 2, device=vol.device)
    out[:, :, :H, :W] = z
    out[:, :, H + 2:, :W] = torch.nn.functional.interpolate(x.permute(0, 1, 3, 2), size=[s, H], mode="nearest")
    out[:, :, :H, W + 2:] = torch.nn.functional.interpolate(y, size=[H, s], mode="nearest")
    return out


def torch_evaluate_step(gt, pred, step, mean, std, ths=0.05):
    g = (gt / 2 ** step) * std - mean
    p = (pred / 2 ** step) * std - mean
    pm = p.clone()
    pm[pm < pm.abs().max() * ths] = 0
    mae = (g - pm).abs().mean() * 100
    psnr = 20 * torch.log10(1.0 / torch.sqrt(torch.mean((g - p) ** 2)))
    return float(psnr), float(mae), torch_projection(p), torch_projection(g), torch_projection((p - g).abs())


def entry(t, nbytes):
    med, lo, hi = t
    return {"ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes": int(nbytes), "GBps": round(nbytes / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_time.json"))
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--once", action="store_true", help="a few evaluate_step calls and nothing else (the profiled child)")
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    H = W = 512
    levels = [96 // 2 ** n for n in range(5)]
    gts = [torch.randn(1, D, H, W, generator=g).cuda() for D in levels]
    preds = [(gt + 0.1 * torch.randn(1, 1, H, W, generator=g).cuda()) for gt in gts]
    if a.once:
        for _ in range(3):
            for n in range(5):
                CWFA.evaluate_step(gts[n], preds[n], n, MEAN, STD, on_device=True)
        torch.cuda.synchronize()
        return
    out = {"workload": "evaluation of one 512x512x96 volume (B=1), pyramid levels D = 96, 48, 24, 12, 6", "repeats": a.repeats,
           "note": "ms = median (min, max) of HIP-event times, the rows of one block measured alternating in one process; bytes algorithmic"}
    gt, pred = gts[0], preds[0]
    n_bytes = gt.numel() * 4
    aff = ops.eval_affine(STEP, MEAN, STD)
    thr = float(ops.volume_extrema(pred, gt, aff).cpu()[0, 3]) * 0.05
    zp, xp, yp, _ = ops.mip3(pred)
    fill = ops.volume_extrema(zp.reshape(1, 1, 1, -1))[0, 0:1]
    t = alternate({
        "evaluate_step": lambda: CWFA.evaluate_step(gt, pred, STEP, MEAN, STD, on_device=True),
        "torch_evaluate_step": lambda: torch_evaluate_step(gt, pred, STEP, MEAN, STD),
        "sample_stats": lambda: ops.sample_stats(gt),
        "volume_extrema_2": lambda: ops.volume_extrema(pred, gt, aff),
        "volume_extrema_1": lambda: ops.volume_extrema(pred, None, aff),
        "volume_metrics": lambda: ops.volume_metrics(pred, gt, thr, aff),
        "mip3_triple": lambda: ops.mip3(pred, gt, triple=True, affine=aff),
        "mip3_single": lambda: ops.mip3(pred, affine=aff),
        "projection_compose": lambda: ops.projection_compose(zp, xp, yp, fill),
        "select_positive": lambda: ops.select_positive(gt),
    }, a.repeats)
    # which of mip3's three reductions bounds it: the three-set kernel with each one dropped in turn ("mip3_ablate", results wrong)
    abl = {}
    for name, mask in (("all", 0), ("no_over_depth", 1), ("no_over_H", 2), ("no_over_W", 4), ("loads_only", 7)):
        ops.set_option("mip3_ablate", mask)
        abl[name] = alternate({"m": lambda: ops.mip3(pred, gt, triple=True, affine=aff)}, a.repeats)["m"]
    ops.set_option("mip3_ablate", 0)
    out["mip3_triple_ablation_ms"] = {k: [round(x, 4) for x in v] for k, v in abl.items()}
    small = (H * W + W * 96 + H * 96) * 4
    nb = {"evaluate_step": 6 * n_bytes, "torch_evaluate_step": 6 * n_bytes, "sample_stats": n_bytes, "volume_extrema_2": 2 * n_bytes,
          "volume_extrema_1": n_bytes, "volume_metrics": 2 * n_bytes, "mip3_triple": 2 * n_bytes + 3 * small, "mip3_single": n_bytes + small,
          "projection_compose": small + (H + 194) * (W + 194) * 4, "select_positive": 4 * n_bytes}
    out["full_size"] = {k: entry(v, nb[k]) for k, v in t.items()}
    out["full_size"]["evaluate_step"]["bytes_note"] = "three passes over (pred, gt): extrema, metrics, projections"
    out["full_size"]["torch_evaluate_step"]["bytes_note"] = "GB/s against the SAME 6 tensor reads; the torch form moves several times that"
    t = alternate({
        "evaluate_step": lambda: [CWFA.evaluate_step(gts[n], preds[n], n, MEAN, STD, on_device=True) for n in range(5)],
        "torch_evaluate_step": lambda: [torch_evaluate_step(gts[n], preds[n], n, MEAN, STD) for n in range(5)],
        "sample_stats": lambda: [ops.sample_stats(gts[n]) for n in range(5)],
    }, a.repeats)
    tot = sum(x.numel() for x in gts) * 4
    out["five_levels"] = {"evaluate_step": entry(t["evaluate_step"], 6 * tot), "torch_evaluate_step": entry(t["torch_evaluate_step"], 6 * tot),
                          "sample_stats": entry(t["sample_stats"], tot)}
    fs = out["full_size"]
    spread = lambda k: fs[k]["ms_max"] - fs[k]["ms_min"]            # noqa: E731
    out["acceptance"] = {
        "evaluate_step_faster_than_torch_by_more_than_spread":
            fs["torch_evaluate_step"]["ms"] - fs["evaluate_step"]["ms"] > max(spread("torch_evaluate_step"), spread("evaluate_step")),
        "speedup_vs_torch_full_size": round(fs["torch_evaluate_step"]["ms"] / fs["evaluate_step"]["ms"], 2),
        "speedup_vs_torch_five_levels": round(out["five_levels"]["torch_evaluate_step"]["ms"] / out["five_levels"]["evaluate_step"]["ms"], 2),
        "sample_stats_GBps_minus_spread": round(n_bytes / fs["sample_stats"]["ms_max"] / 1e6, 1),
        "extrema_reaches_sample_stats": fs["volume_extrema_2"]["GBps"] >= n_bytes / fs["sample_stats"]["ms_max"] / 1e6,
        "metrics_reaches_sample_stats": fs["volume_metrics"]["GBps"] >= n_bytes / fs["sample_stats"]["ms_max"] / 1e6,
    }
    # corr_coeff_3D, T = 32, N = 200 ROIs: wall time, host part included
    T, D = 32, 96
    rs = np.random.RandomState(0)
    sg = torch.rand(T, D, 256, 256, generator=g).cuda()
    sp = (sg * 0.9).contiguous()
    coords = [(int(rs.randint(8, 248)), int(rs.randint(8, 248)), int(rs.randint(0, 25))) for _ in range(200)]
    walls = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        CWFA.corr_coeff_3D(sg, sp, coords, 5, 3, minmax_ths=0.0)
        walls.append((time.perf_counter() - t0) * 1e3)
    dev = alternate({"roi_means_200": lambda: ops.roi_means(sg, CWFA.roi_boxes(coords, sg.shape, 5, 3)),
                     "select_positive": lambda: ops.select_positive(sg), "volume_extrema": lambda: ops.volume_extrema(sg)}, a.repeats)
    out["corr_coeff_3D"] = {"shape": [T, D, 256, 256], "rois": 200, "wall_ms_median_after_first": round(statistics.median(walls[1:]), 2),
                            "device_ms": {k: round(v[0], 4) for k, v in dev.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["acceptance"]))
    if a.kernel_stats:
        rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        with tempfile.TemporaryDirectory() as d:
            subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--once"],
                           check=True, timeout=300)
            hits = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not hits:
                raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
            shutil.copy(hits[0], a.kernel_stats)


if __name__ == "__main__":
    main()
