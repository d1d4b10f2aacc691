#!/usr/bin/env python3
"""Time the demixing of overlapping footprints on the MI355X and write profiles/demix_time.json.

The scene: N = 4096 neurons on a 16 x 16 x 16 lattice of spacing (4, 7, 7) with boxes of 6 x 10 x 10 voxels, so that every box meets
the boxes of its 26 lattice neighbours (fewer at the faces); the footprints are ellipsoids of semi-axes (3, 5, 5) with weights
0.5 + 0.5 exp(-d^2 / 2) jittered by 10 %, as a thresholded correlation looks: of the 26 neighbours whose boxes a box meets, the
footprints of the six along the axes share voxels (the record says how many coefficients are non-zero per row).
T = 10 000 time steps; the traces are F = (I + M) f for planted f >= 0 (sparse activity on a baseline), so the solve has a known
answer.

  * the plan (``CWFA.demix_plan``): host clock around the call and a synchronise, with the host pair enumeration on its own;
  * the solve (``CWFA.demix_traces``, n_sweeps = 64, tol = 0 and tol = 1e-9, nonneg on), HIP events, warmed up, median (min, max)
    over windows, alternating with the yardstick and the torch form in one process;
  * the sweeps-per-step histogram;
  * the bytes it must move -- F read once, Fd written once, 16 N T -- at the rate of a 1 GiB ``Tensor.copy_`` of the same run;
  * the torch form of the unconstrained problem: a dense float64 ``torch.linalg.solve(I + M, F)``, with the largest difference from
    the library's ``nonneg=False`` result and from the planted f;
  * ``bench.py --gpus 1 --steps 20 --warmup 3`` of this tree, and of the tree given with ``--parent DIR``, each in a fresh process.
    python tools/demix_time.py [--quick] [--parent DIR]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402

SPACING, R = (4, 7, 7), (3, 5, 5)


def footprints(side, gen):
    """``CWFA.Footprints`` of side^3 neurons on the lattice, made on the host: ellipsoids inside the boxes."""
    import numpy as np
    import torch
    from cwfa_amd import CWFA
    k = np.arange(side)
    z, y, x = np.meshgrid(R[0] + SPACING[0] * k, R[1] + SPACING[1] * k, R[2] + SPACING[2] * k, indexing="ij")
    c = np.stack([z.ravel(), y.ravel(), x.ravel()], axis=1)
    boxes = np.stack([c[:, 0] - R[0], c[:, 0] + R[0], c[:, 1] - R[1], c[:, 1] + R[1], c[:, 2] - R[2], c[:, 2] + R[2]], axis=1).astype(np.int32)
    N, vox = len(boxes), 8 * R[0] * R[1] * R[2]
    dz, dy, dx = np.meshgrid(*(np.arange(-r, r) + 0.5 for r in R), indexing="ij")
    inside = (dz / R[0]) ** 2 + (dy / R[1]) ** 2 + (dx / R[2]) ** 2 <= 1.0
    profile = np.where(inside, 0.5 + 0.5 * np.exp(-0.5 * ((dz / 1.2) ** 2 + (dy / 2.0) ** 2 + (dx / 2.0) ** 2)), 0.0).ravel()
    w = torch.tensor(profile, dtype=torch.float32, device="cuda")[None, :] * (0.9 + 0.1 * torch.rand(N, vox, device="cuda", generator=gen))
    w = torch.where(w >= 0.5, w, torch.zeros_like(w)).reshape(-1).contiguous()
    wsum = w.reshape(N, vox).double().sum(1)
    sizes = (w.reshape(N, vox) > 0).sum(1).to(torch.int32)
    offsets = (np.arange(N + 1, dtype=np.int64) * vox)
    return CWFA.Footprints(boxes, offsets, w, wsum, sizes, w)


def bench_line(tree):
    """The JSON line of ``bench.py --gpus 1 --steps 20 --warmup 3`` run in ``tree`` by a fresh process."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=tree, capture_output=True, text=True,
                       timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]) if r.returncode == 0 and lines else {"failed": r.returncode, "stderr": r.stderr[-400:]}


def measure(quick):
    import numpy as np
    import torch
    from cwfa_amd import CWFA, ops
    side, T = (6, 1000) if quick else (16, 10000)
    gen = torch.Generator(device="cuda").manual_seed(7)
    fp = footprints(side, gen)
    N = len(fp.boxes)
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        pairs = ops.footprint_pairs(fp.boxes)
        host.append(1e3 * (time.perf_counter() - t0))
    whole = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = CWFA.demix_plan(fp)
        torch.cuda.synchronize()
        whole.append(1e3 * (time.perf_counter() - t0))
    val = plan.val.cpu().numpy()
    rows = np.repeat(np.arange(N), np.diff(plan.rowptr))
    nonzero = np.bincount(rows[val != 0], minlength=N)
    rowsum = np.bincount(rows, weights=val, minlength=N)
    A = torch.eye(N, dtype=torch.float64, device="cuda")
    A[torch.tensor(rows).cuda(), torch.tensor(plan.col.astype(np.int64)).cuda()] = plan.val
    f = 1.0 + 4.0 * torch.rand(N, T, dtype=torch.float64, device="cuda", generator=gen) * (
        torch.rand(N, T, device="cuda", generator=gen) < 0.1)
    F = A @ f
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=gen), torch.empty(n_copy, device="cuda")
    fns = {"solve_tol0": lambda: CWFA.demix_traces(F, plan, 64, 0.0, True), "solve_tol1e-9": lambda: CWFA.demix_traces(F, plan, 64, 1e-9, True),
           "float4_copy": lambda: dst.copy_(src), "torch_linalg_solve": lambda: torch.linalg.solve(A, F)}
    nbytes = {"solve_tol0": 16 * N * T, "solve_tol1e-9": 16 * N * T, "float4_copy": 8 * n_copy}
    ms = windows(fns, 3 if quick else 7, 1, 1 if quick else 2)
    r = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    rate = r["float4_copy"]["GBps"]
    res = {}
    for k, tol in (("solve_tol0", 0.0), ("solve_tol1e-9", 1e-9)):
        Fd, sweeps = CWFA.demix_traces(F, plan, 64, tol, True)
        s = sweeps.cpu().numpy()
        r[k]["floor_ms_at_measured_copy_rate"] = round(nbytes[k] / rate / 1e6, 5)
        r[k]["multiple_of_floor"] = round(r[k]["ms"] / r[k]["floor_ms_at_measured_copy_rate"], 1)
        r[k]["torch_form_over_this"] = round(r["torch_linalg_solve"]["ms"] / r[k]["ms"], 2)
        r[k]["sweeps_histogram"] = {str(v): int(c) for v, c in zip(*np.unique(s, return_counts=True))}
        r[k]["bytes_swept"] = int(s.sum()) * (8 * (len(plan.col) + 2 * N))       # per sweep and step: a read per entry, F and f per row
        r[k]["largest_difference_from_the_planted_f"] = float((Fd - f).abs().max())
    free = CWFA.demix_traces(F, plan, 64, 0.0, False)[0]
    dense = torch.linalg.solve(A, F)
    res["unconstrained"] = {"library_minus_linalg_solve_max": float((free - dense).abs().max()),
                            "linalg_solve_minus_planted_max": float((dense - f).abs().max()), "largest_F": float(F.abs().max())}
    res["plan"] = {"host_pairs_ms": summary(host), "demix_plan_ms_host_clock_with_synchronise": summary(whole)}
    res["times"] = r
    res["config"] = {"neurons": N, "time_steps": T, "lattice_spacing": list(SPACING), "box": [2 * v for v in R], "pairs": len(plan.pairs),
                     "entries": len(plan.col), "neighbours_per_row_min_median_max": [int(np.diff(plan.rowptr).min()),
                                                                                   float(np.median(np.diff(plan.rowptr))), int(np.diff(plan.rowptr).max())],
                     "nonzero_coefficients_per_row_min_median_max": [int(nonzero.min()), float(np.median(nonzero)), int(nonzero.max())],
                     "coefficient_max": float(val.max()), "row_sum_max": float(rowsum.max()),
                     "footprint_sizes_min_median_max": [int(fp.sizes.min()), float(fp.sizes.double().median()), int(fp.sizes.max())],
                     "copy_elements": n_copy}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "demix_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "demixing of overlapping footprints: the plan, the projected Gauss-Seidel solve, and a dense torch.linalg.solve",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time, the forms alternating in one process; the plan by "
                       "the host clock around the call and a synchronise",
           "box": device_record(), "demix": measure(quick)}
    torch.cuda.empty_cache()
    print(json.dumps(rec["demix"]), flush=True)
    if not quick:
        rec["bench"] = {"this_tree": bench_line(ROOT)}
        print(json.dumps(rec["bench"]), flush=True)
        if "--parent" in sys.argv:
            rec["bench"]["parent_tree"] = bench_line(os.path.abspath(sys.argv[sys.argv.index("--parent") + 1]))
    rec["not_measured"] = ["hardware counters of the three kernels", "an LDS-staged form of the solve (not built)",
                           "footprints of a real recording", "N or T other than the ones above"]
    out = os.path.join(ROOT, "profiles", "demix_time_quick.json" if quick else "demix_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec.get("bench")))


if __name__ == "__main__":
    main()
