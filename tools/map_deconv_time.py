#!/usr/bin/env python3
"""Time MAP Richardson-Lucy against the plain loop on the problem of tools/accel_deconv_time.py (object 600,
PSF 2160, 120 depths: full size 2760, all depths in one FFT batch; the synthetic lenslet PSF and sparse object described there) in
one process.  The prior is the true object plus noise of the prior's own width: sigma = 0.2 * object + 20, mean = object + sigma *
N(0, 1) from a fixed seed (it is negative in places), weight 1.
Measured, each three times (the spread is reported, the variants alternate):
  per iteration  tools/deconv_time.py's difference method: (call of 1 + K iterations - call of 1 iteration) / K after a warm-up call,
                 for the plain loop (the code the parent commit runs), the loop with the prior, with the prior and the objective
                 trace, and the accelerated loop with both;
  kernels        update and update_accel (the siblings, same run), update_map, update_accel_map (with and without the penalty
                 reduction) and penalty alone with HIP events, against the bytes each has to move;
  convergence    descriptive: the objective trace of 101 iterations with the prior from ones and of 101 from init = max(mean, 0.01);
                 the first k from init whose objective is at or below that of 100 iterations from ones; the distance of the results
                 from the true object.
Writes one JSON file.
    python tools/map_deconv_time.py [--obj 600] [--psf 2160] [--depths 120] [--out profiles/map_deconv_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cwfa_amd import ops, utils as U   # noqa: E402

from accel_deconv_time import lenslet_psf, spread  # noqa: E402
from deconv_time import event_ms, per_iteration  # noqa: E402

REPEATS = 3


def make_problem(a):
    """accel_deconv_time.make_problem with the same seed and draws, keeping the object: (OTF, img, object, stats)."""
    g = torch.Generator(device="cuda").manual_seed(2020)
    D, P, obj = a.depths, a.psf, a.obj
    psf = lenslet_psf(D, P, "cuda")
    vol = torch.rand(1, D, obj, obj, generator=g, device="cuda")
    vol = torch.where(vol > 0.9995, (vol - 0.9995) * 8e6 + 2000, torch.zeros((), device="cuda"))
    clean, OTF = U.fft_conv_split(vol, psf, [P, P], n_split=max(1, D // 10))
    del psf
    img = torch.poisson(clean + a.background, generator=g)
    stats = {"mean_counts": float(img.mean()), "max_counts": float(img.max()), "background": a.background}
    return OTF, img.contiguous(), vol, stats


def make_prior(vol):
    g = torch.Generator(device="cuda").manual_seed(7)
    sigma = 0.2 * vol + 20.0
    mean = vol + sigma * torch.randn(vol.shape, generator=g, device="cuda")
    return mean.contiguous(), sigma.contiguous(), mean.clamp(min=0.01).contiguous()


def kernel_table(a):
    D, F, obj = a.depths, a.obj + a.psf, a.obj
    po = a.psf // 2
    g = torch.Generator(device="cuda").manual_seed(1)
    objp = torch.zeros(1, D, F, F, device="cuda")
    objp[:, :, po:po + obj, po:po + obj] = torch.rand(1, D, obj, obj, generator=g, device="cuda")
    real = torch.rand(1, D, F, F, generator=g, device="cuda") + 0.5
    gs, xn, mu, w = (torch.rand(1, D, obj, obj, generator=g, device="cuda") for _ in range(4))
    w *= 2.0                                                                             # w mu on both sides of 1
    slab, pen = ops.deconv_accel_slab(D, obj, "cuda"), ops.deconv_penalty_slab(D, obj, "cuda")
    trace = torch.zeros(1, dtype=torch.float64, device="cuda")
    n = 4 * D * obj * obj

    def reset():                                                                         # the in-place forms would decay to 0 or grow
        objp[:, :, po:po + obj, po:po + obj] = 1.0

    rows = {
        "update (the sibling)": (lambda: ops.deconv_update(objp, real, obj, po), 3 * n),
        "update_map": (lambda: ops.deconv_update_map(objp, real, mu, w, obj, po), 5 * n),
        "update_map, with the penalty": (lambda: ops.deconv_update_map(objp, real, mu, w, obj, po, pen), 5 * n),
        "update_accel (the sibling)": (lambda: ops.deconv_update_accel(objp, real, gs, xn, slab, obj, po), 5 * n),
        "update_accel_map": (lambda: ops.deconv_update_accel_map(objp, real, gs, xn, mu, w, slab, obj, po), 7 * n),
        "update_accel_map, with the penalty": (lambda: ops.deconv_update_accel_map(objp, real, gs, xn, mu, w, slab, obj, po, pen), 7 * n),
        "penalty": (lambda: ops.deconv_penalty(pen, trace, 0), 2 * 8 * pen.numel()),
    }
    out = {}
    for name, (fn, nbytes) in rows.items():
        ms = []
        for _ in range(REPEATS):
            reset()
            ms.append(event_ms(fn))
        out[name] = {"ms": spread(ms), "bytes": nbytes, "GBps": spread([nbytes / m / 1e6 for m in ms])}
    out["penalty"]["rows"] = pen.numel()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj", type=int, default=600)
    ap.add_argument("--psf", type=int, default=2160)
    ap.add_argument("--depths", type=int, default=120)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--plain-iterations", type=int, default=100)
    ap.add_argument("--background", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_deconv_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "map_deconv_time.py needs the MI355X"
    torch.set_grad_enabled(False)
    OTF, img, vol, stats = make_problem(a)
    mean, sigma, init = make_prior(vol)
    kw = dict(ObjSize=[a.obj, a.obj], PSFShape=[a.psf, a.psf], ROIsize=[a.obj, a.obj, a.depths])
    pr = dict(prior_mean=mean, prior_std=sigma)
    variants = {"plain": {}, "prior": pr, "prior_with_trace": dict(pr, trace=True),
                "prior_accelerated_with_trace": dict(pr, trace=True, accelerate=True)}
    per = {k: [] for k in variants}
    for _ in range(REPEATS):
        for name, more in variants.items():
            per[name].append(per_iteration(lambda n: U.XLFMDeconv(OTF, img, n, **kw, **more), a.iters)[0])
        torch.cuda.empty_cache()
    N = a.plain_iterations
    rms = lambda v: float(((v - vol).double() ** 2).mean().sqrt())
    plain = U.XLFMDeconv(OTF, img, N, **kw)[0]
    dist = {"plain_from_ones": rms(plain), "prior_mean_itself": rms(mean)}
    del plain
    out = U.XLFMDeconv(OTF, img, N + 1, trace=True, **kw, **pr)
    ones, dist["prior_from_ones"] = out[3], rms(out[0])
    out = U.XLFMDeconv(OTF, img, N + 1, trace=True, init=init, **kw, **pr)
    warm, dist["prior_from_init"] = out[3], rms(out[0])
    del out
    torch.cuda.empty_cache()
    target = ones[N]
    reached = next((k for k, v in enumerate(warm) if v <= target), None)
    marks = [k for k in (0, 1, 2, 5, 10, 20, 30, 50, 100) if k <= N]
    res = {"shape": {"object": a.obj, "psf": a.psf, "depths": a.depths, "full": a.obj + a.psf, "n_split_fourier": 1},
           "problem": dict(stats, prior="sigma = 0.2 object + 20, mean = object + sigma N(0, 1), weight 1, init = max(mean, 0.01)",
                           share_of_second_branch=float((mean / (sigma * sigma) >= 1).float().mean()),
                           share_of_negative_means=float((mean < 0).float().mean())),
           "repeats": REPEATS, "iterations_timed": a.iters,
           "ms_per_iteration": {k: spread(v) for k, v in per.items()},
           "convergence": {"iterations_from_ones": N, "objective_after_them": target, "iterations_from_init_to_reach_it": reached,
                           "rises_from_ones": sum(1 for p, q in zip(ones, ones[1:]) if q > p),
                           "rises_from_init": sum(1 for p, q in zip(warm, warm[1:]) if q > p),
                           "objective_after_k_iterations": {str(k): {"from_ones": ones[k], "from_init": warm[k]} for k in marks},
                           "rms_distance_from_the_true_object": dist},
           "kernels": kernel_table(a)}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
