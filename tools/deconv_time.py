#!/usr/bin/env python3
"""Time the Richardson-Lucy deconvolution at the reference's size (object 600, PSF 2160, 120 depths: full size 2760) in one process:
  fused:  cwfa_amd.utils.XLFMDeconv -- rocFFT plus the kernels of csrc/deconv_ops.hip;
  torch:  the operator-by-operator restatement of tests/deconv_ref.py on the same card, which is the reference's own sequence of
          torch operators (pad, rfft2, product, irfft2, two rolls, relu, sum, ..., median over a masked copy, clamp, negative pad).
Both are called with 1 iteration (warm-up: FFT plans, code objects) and then with 1 and with 1 + K iterations; the time per
iteration is the difference over K (K = 3), so the allocation and set-up of a call cancel out.  Every call ends in a device
synchronise (the loop reads a flag back per iteration anyway).
Then each new kernel alone at that shape with HIP events, against the bytes it has to move and the 8000 GB/s DESIGN.md uses.
With --profile-only one fused call of 2 iterations runs on a random transfer function and image (no FFT outside that call) and
nothing is timed: for `rocprofv3 --kernel-trace --stats -- python tools/deconv_time.py --profile-only`, which gives the FFT kernels'
share of the call.  Writes one JSON file.
    python tools/deconv_time.py [--obj 600] [--psf 2160] [--depths 120] [--out profiles/deconv_time.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cwfa_amd import ops, utils as U   # noqa: E402

import deconv_ref as R  # noqa: E402

PEAK_GBPS = 8000.0


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, steps=5):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def make_problem(a):
    """A sparse PSF, its OTF (computed per depth chunk through the package's own fft_conv_split) and a noisy image of a sparse volume."""
    g = torch.Generator(device="cuda").manual_seed(2525)
    D, P, obj = a.depths, a.psf, a.obj
    psf = torch.rand(1, D, P, P, generator=g, device="cuda") ** 6
    psf /= psf.sum((2, 3), keepdim=True)
    vol = torch.rand(1, D, obj, obj, generator=g, device="cuda")
    vol = torch.where(vol > 0.85, vol, torch.zeros((), device="cuda")) * 25
    img, OTF = U.fft_conv_split(vol, psf, [P, P], n_split=max(1, D // 10))
    img = img + 0.05 * img.mean() * torch.randn(img.shape, generator=g, device="cuda")
    del psf, vol
    return OTF, img.contiguous()


def per_iteration(call, K):
    call(1)                                                             # warm-up
    t1, _ = wall_ms(lambda: call(1))
    tk, out = wall_ms(lambda: call(1 + K))
    return (tk - t1) / K, t1, tk, out


def kernel_table(a, OTF):
    D, F = a.depths, a.obj + a.psf
    Fh, po = F // 2 + 1, a.psf // 2
    g = torch.Generator(device="cuda").manual_seed(1)
    spec = torch.view_as_complex(torch.randn(1, D, F, Fh, 2, generator=g, device="cuda"))
    one = torch.view_as_complex(torch.randn(1, 1, F, Fh, 2, generator=g, device="cuda"))
    real = torch.randn(1, D, F, F, generator=g, device="cuda")
    objp = torch.zeros(1, D, F, F, device="cuda")
    plane, est = torch.randn(1, 1, F, F, generator=g, device="cuda"), torch.rand(1, 1, F, F, generator=g, device="cuda")
    tmp, flag = torch.empty_like(plane), torch.zeros(1, dtype=torch.int32, device="cuda")
    med = ops.select_nonzero(plane)
    ws = torch.empty(U._lib.SELECT_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda")
    cplx, pl = 8 * D * F * Fh, 4 * F * F
    rows = {
        "spectrum_mul (forward, in place)": (lambda: ops.deconv_spectrum_mul(spec, OTF, out=spec), 3 * cplx),
        "spectrum_mul (backward, broadcast, conj)": (lambda: ops.deconv_spectrum_mul(one, OTF, conj=True, out=spec), 2 * cplx + 8 * F * Fh),
        "project (relu, depth sum)": (lambda: ops.deconv_project(real, out=est, pre="relu"), D * pl + pl),
        "ratio": (lambda: ops.deconv_ratio(plane, est, tmp, flag), 3 * pl),
        "select_nonzero (4 passes)": (lambda: ops.select_nonzero(plane, out=med, workspace=ws), 4 * pl),
        "clamp": (lambda: ops.deconv_clamp(tmp, med[0], med[1], 10), 2 * pl),
        "update (window only)": (lambda: ops.deconv_update(objp, real, a.obj, po), 3 * 4 * D * a.obj * a.obj),
    }
    out = {}
    for name, (fn, nbytes) in rows.items():
        ms = event_ms(fn)
        out[name] = {"ms": round(ms, 4), "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1), "share_of_hbm_peak": round(nbytes / ms / 1e6 / PEAK_GBPS, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj", type=int, default=600)
    ap.add_argument("--psf", type=int, default=2160)
    ap.add_argument("--depths", type=int, default=120)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--n-split-fourier", type=int, default=1)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deconv_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "deconv_time.py needs the MI355X"
    torch.set_grad_enabled(False)
    if a.profile_only:                                                  # no FFT outside the traced call: contents do not matter to a trace
        g = torch.Generator(device="cuda").manual_seed(2525)
        F = a.obj + a.psf
        OTF = torch.view_as_complex(torch.randn(1, a.depths, F, F // 2 + 1, 2, generator=g, device="cuda") * 1e-3)
        img = torch.rand(1, 1, a.psf, a.psf, generator=g, device="cuda") + 0.5
    else:
        OTF, img = make_problem(a)
    kw = dict(ObjSize=[a.obj, a.obj], PSFShape=[a.psf, a.psf], ROIsize=[a.obj, a.obj, a.depths], n_split_fourier=a.n_split_fourier)
    if a.profile_only:
        U.XLFMDeconv(OTF, img, 2, **kw)
        torch.cuda.synchronize()
        return
    fused_ms, f1, fk, fused = per_iteration(lambda n: U.XLFMDeconv(OTF, img, n, **kw), a.iters)
    vol_f, est_f = fused[0].clone(), fused[2].clone()
    del fused
    torch.cuda.empty_cache()
    torch_ms, t1, tk, ref = per_iteration(lambda n: R.xlfm_deconv(OTF, img, n, kw["ObjSize"], kw["ROIsize"], a.n_split_fourier, 10), a.iters)
    agree = {"volume_max_rel_difference": float((vol_f - ref[0]).abs().max() / ref[0].abs().max()),
             "estimate_max_rel_difference": float((est_f - ref[1]).abs().max() / ref[1].abs().max())}
    del ref, vol_f, est_f
    torch.cuda.empty_cache()
    res = {"shape": {"object": a.obj, "psf": a.psf, "depths": a.depths, "full": a.obj + a.psf, "n_split_fourier": a.n_split_fourier},
           "iterations_timed": a.iters,
           "fused": {"ms_per_iteration": round(fused_ms, 2), "call_1_iteration_ms": round(f1, 2), f"call_{1 + a.iters}_iterations_ms": round(fk, 2),
                     "seconds_per_100_iterations": round(fused_ms / 10, 2)},
           "torch_restatement": {"ms_per_iteration": round(torch_ms, 2), "call_1_iteration_ms": round(t1, 2),
                                 f"call_{1 + a.iters}_iterations_ms": round(tk, 2), "seconds_per_100_iterations": round(torch_ms / 10, 2)},
           "agreement_after_%d_iterations" % (1 + a.iters): agree, "peak_GBps_assumed": PEAK_GBPS, "kernels": kernel_table(a, OTF)}
    res["kernels_ms_per_iteration_sum"] = round(sum(v["ms"] for v in res["kernels"].values()), 3)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
