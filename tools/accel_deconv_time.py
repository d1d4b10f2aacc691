#!/usr/bin/env python3
"""Time the accelerated Richardson-Lucy loop against the plain one at the reference's size (object 600, PSF 2160,
120 depths: full size 2760, all depths in one FFT batch) in one process, on a synthetic lenslet problem:
  PSF    a square grid of Gaussian spots whose pitch grows with depth (the pattern shears about the centre) and whose width grows away
         from the middle depth, every depth normalised -- not a random transfer function, and not a recorded one either;
  image  the forward projection of a sparse object (through the package's own fft_conv_split, which also gives the OTF) plus a
         background, Poisson-noised from a fixed seed.
Measured, each three times (the spread is reported, plain and accelerated alternate):
  per iteration  tools/deconv_time.py's difference method: (call of 1 + K iterations - call of 1 iteration) / K after a warm-up call;
  kernels        update (the sibling yardstick), update_accel, alpha, predict, poisson_nll alone with HIP events, against the bytes
                 each has to move;
  convergence    the likelihood trace of 101 plain and 101 accelerated iterations (trace[k] belongs to the state after k
                 iterations), the first accelerated k whose likelihood is at or below the plain loop's after 100, and the wall time of
                 a plain call of 100 and an accelerated call of that many iterations.
Writes one JSON file.  With --working-set-only it times the three window kernels at fewer depths instead (a launch's distinct bytes
against the 256 MiB Infinity Cache) and writes <out>_working_set.json.
    python tools/accel_deconv_time.py [--obj 600] [--psf 2160] [--depths 120] [--out profiles/accel_deconv_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cwfa_amd import ops, utils as U   # noqa: E402

from deconv_time import event_ms, per_iteration, wall_ms  # noqa: E402

REPEATS = 3


def lenslet_psf(D, P, device, pitch=0.125, shear=0.002, sigma0=1.6, widen=0.05):
    """[1, D, P, P]: spots on a square grid of ``pitch`` * P pixels at the middle depth, the grid scaled by 1 + shear * dz about the
    centre, Gaussian spots of sigma0 + widen * |dz| pixels; a grid of separable spots is the outer product of two 1-D profiles."""
    x = torch.arange(P, dtype=torch.float64, device=device) - (P - 1) / 2
    k = torch.arange(-3, 5, dtype=torch.float64, device=device) - 0.5                    # 8 x 8 lenslets
    psf = torch.empty(1, D, P, P, dtype=torch.float32, device=device)
    for z in range(D):
        dz = z - (D - 1) / 2
        centres = k * pitch * P * (1 + shear * dz)
        sig = sigma0 + widen * abs(dz)
        u = torch.exp(-(x[:, None] - centres[None, :]) ** 2 / (2 * sig * sig)).sum(1)
        u /= u.sum()
        psf[0, z] = torch.outer(u, u).float()
    return psf


def make_problem(a):
    g = torch.Generator(device="cuda").manual_seed(2020)
    D, P, obj = a.depths, a.psf, a.obj
    psf = lenslet_psf(D, P, "cuda")
    vol = torch.rand(1, D, obj, obj, generator=g, device="cuda")
    vol = torch.where(vol > 0.9995, (vol - 0.9995) * 8e6 + 2000, torch.zeros((), device="cuda"))    # 1 voxel in 2000, 2000 .. 6000
    clean, OTF = U.fft_conv_split(vol, psf, [P, P], n_split=max(1, D // 10))
    del psf, vol
    img = torch.poisson(clean + a.background, generator=g)
    stats = {"mean_counts": float(img.mean()), "max_counts": float(img.max()), "background": a.background}
    return OTF, img.contiguous(), stats


def spread(values):
    v = sorted(values)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def kernel_table(a):
    D, F, obj = a.depths, a.obj + a.psf, a.obj
    po = a.psf // 2
    g = torch.Generator(device="cuda").manual_seed(1)
    objp = torch.zeros(1, D, F, F, device="cuda")
    objp[:, :, po:po + obj, po:po + obj] = torch.rand(1, D, obj, obj, generator=g, device="cuda")
    real = torch.rand(1, D, F, F, generator=g, device="cuda") + 0.5
    gs, xn, xp = (torch.rand(1, D, obj, obj, generator=g, device="cuda") for _ in range(3))
    slab, alpha = ops.deconv_accel_slab(D, obj, "cuda"), torch.zeros(1, device="cuda")
    est, img = torch.rand(1, 1, F, F, generator=g, device="cuda") + 0.5, torch.rand(1, 1, F, F, generator=g, device="cuda")
    trace, ws = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.empty(U._lib.DECONV_NLL_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda")
    w = 4 * D * obj * obj
    rows = {
        "update (window only)": (lambda: ops.deconv_update(objp, real, obj, po), 3 * w),
        "update_accel": (lambda: ops.deconv_update_accel(objp, real, gs, xn, slab, obj, po), 5 * w),
        "alpha": (lambda: ops.deconv_alpha(slab, 0.999, alpha), 2 * slab.numel() * 8),
        "predict": (lambda: ops.deconv_predict(objp, xn, xp, alpha, obj, po), 3 * w),
        "poisson_nll": (lambda: ops.deconv_poisson_nll(img, est, trace, 0, ws), 2 * 4 * F * F),
    }
    out = {}
    for name, (fn, nbytes) in rows.items():
        ms = [event_ms(fn) for _ in range(REPEATS)]
        out[name] = {"ms": spread(ms), "bytes": nbytes, "GBps": spread([nbytes / m / 1e6 for m in ms])}
    return out


def working_set_table(a):
    """update, update_accel and predict at the full window and fewer depths: the GB/s of repeated launches against the distinct bytes
    a launch touches, which the 256 MiB Infinity Cache keeps from one launch to the next while they fit."""
    F, obj, po = a.obj + a.psf, a.obj, a.psf // 2
    out = {}
    for D in sorted({max(1, a.depths * k // 15) for k in (2, 4, 6, 10, 15)}):
        g = torch.Generator(device="cuda").manual_seed(1)
        objp = torch.zeros(1, D, F, F, device="cuda")
        objp[:, :, po:po + obj, po:po + obj] = torch.rand(1, D, obj, obj, generator=g, device="cuda")
        real = torch.rand(1, D, F, F, generator=g, device="cuda") + 0.5
        gs, xn, xp = (torch.rand(1, D, obj, obj, generator=g, device="cuda") for _ in range(3))
        slab, alpha = ops.deconv_accel_slab(D, obj, "cuda"), torch.zeros(1, device="cuda")
        w = 4 * D * obj * obj
        rows = {"update": (lambda: ops.deconv_update(objp, real, obj, po), 3 * w, 2 * w),          # name: launch, bytes moved, distinct bytes
                "update_accel": (lambda: ops.deconv_update_accel(objp, real, gs, xn, slab, obj, po), 5 * w, 4 * w),
                "predict": (lambda: ops.deconv_predict(objp, xn, xp, alpha, obj, po), 3 * w, 3 * w)}
        for name, (fn, nbytes, distinct) in rows.items():
            ms = [event_ms(fn, steps=20) for _ in range(REPEATS)]
            out[f"{name}, {D} depths"] = {"distinct_MB": round(distinct / 1e6), "ms": spread(ms), "GBps": spread([nbytes / m / 1e6 for m in ms])}
        del objp, real, gs, xn, xp
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj", type=int, default=600)
    ap.add_argument("--psf", type=int, default=2160)
    ap.add_argument("--depths", type=int, default=120)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--plain-iterations", type=int, default=100)
    ap.add_argument("--background", type=float, default=2.0)
    ap.add_argument("--working-set-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accel_deconv_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "accel_deconv_time.py needs the MI355X"
    torch.set_grad_enabled(False)
    if a.working_set_only:
        res = {"shape": {"object": a.obj, "psf": a.psf, "full": a.obj + a.psf}, "repeats": REPEATS, "launches_timed": 20, "kernels": working_set_table(a)}
        print(json.dumps(res, indent=1))
        with open(a.out.replace(".json", "_working_set.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    OTF, img, stats = make_problem(a)
    kw = dict(ObjSize=[a.obj, a.obj], PSFShape=[a.psf, a.psf], ROIsize=[a.obj, a.obj, a.depths])
    per = {"plain": [], "accelerated": [], "accelerated_with_trace": []}
    for _ in range(REPEATS):
        per["plain"].append(per_iteration(lambda n: U.XLFMDeconv(OTF, img, n, **kw), a.iters)[0])
        per["accelerated"].append(per_iteration(lambda n: U.XLFMDeconv(OTF, img, n, accelerate=True, **kw), a.iters)[0])
        per["accelerated_with_trace"].append(per_iteration(lambda n: U.XLFMDeconv(OTF, img, n, accelerate=True, trace=True, **kw), a.iters)[0])
        torch.cuda.empty_cache()
    N = a.plain_iterations
    plain = U.XLFMDeconv(OTF, img, N + 1, trace=True, **kw)[3]
    fast = U.XLFMDeconv(OTF, img, N + 1, accelerate=True, trace=True, **kw)[3]
    torch.cuda.empty_cache()
    target = plain[N]
    reached = next((k for k, v in enumerate(fast) if v <= target), None)
    wall_plain = [wall_ms(lambda: U.XLFMDeconv(OTF, img, N, **kw))[0] for _ in range(REPEATS)]
    wall_fast = [wall_ms(lambda: U.XLFMDeconv(OTF, img, reached, accelerate=True, **kw))[0] for _ in range(REPEATS)] if reached else None
    marks = [k for k in (0, 1, 2, 5, 10, 15, 20, 25, 30, 40, 50, 60, 80, 100) if k <= N]
    res = {"shape": {"object": a.obj, "psf": a.psf, "depths": a.depths, "full": a.obj + a.psf, "n_split_fourier": 1},
           "problem": dict(stats, psf="8 x 8 Gaussian spots, pitch 0.125 of the PSF size scaled by 1 + 0.002 dz, sigma 1.6 + 0.05 |dz| pixels",
                           object="1 voxel in 2000 at 2000 .. 6000, Poisson noise from a fixed seed"),
           "repeats": REPEATS, "iterations_timed": a.iters,
           "ms_per_iteration": {k: spread(v) for k, v in per.items()},
           "convergence": {"plain_iterations": N, "plain_nll_after_them": target, "accelerated_iterations_to_reach_it": reached,
                           "accelerated_rises": sum(1 for p, q in zip(fast, fast[1:]) if q > p),
                           "plain_rises": sum(1 for p, q in zip(plain, plain[1:]) if q > p),
                           "nll_after_k_iterations": {str(k): {"plain": plain[k], "accelerated": fast[k]} for k in marks},
                           "wall_ms_plain": spread(wall_plain), "wall_ms_accelerated": spread(wall_fast) if wall_fast else None},
           "kernels": kernel_table(a)}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
