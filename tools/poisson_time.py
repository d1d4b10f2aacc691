#!/usr/bin/env python3
"""Time the shot-noise simulation on the MI355X and write profiles/poisson_time.json.

  * ``ops.rand_poisson`` at 2160 x 2160 (one frame) and at 250 x 2160 x 2160 (a dataset), every sample with its own rates, for rate
    3 (inversion only), 37.5 and 1024 (PTRS only), the mixed input of the tests, and a synthetic frame (sparse blurred spots on a dim
    background) scaled to 32^2 photons at its maximum;
  * ``torch.poisson`` on the same tensors on the same card -- what the library's users had before;
  * a float4 copy of 1 GiB, the yardstick for what a streaming kernel reaches from HBM; the draw has to move 8 bytes per element;
  * the histogram of PTRS attempts of each input, from the restatement (tests/poisson_ref.py) on a 2^16-element subsample;
  * ``XLFMForward`` at 120 x 600^2 under a 2160^2 PSF (full size 2760), the forward half of the deconvolution's iteration.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.  ``--profile-only`` issues every form once, in the order printed, for a kernel trace taken in a run of its own.
    python tools/poisson_time.py [--quick] [--profile-only]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from posterior_time import device_record, summary, windows      # noqa: E402

SEED = 20251019


def frame(S, g):
    """A synthetic lenslet-like frame: sparse spots blurred to a few pixels over a dim background, maximum 1."""
    import torch
    import torch.nn.functional as F
    x = torch.rand(1, 1, S, S, device="cuda", generator=g)
    x = torch.where(x > 0.999, x, torch.zeros((), device="cuda"))
    for _ in range(3):
        x = F.avg_pool2d(x, 5, 1, 2)
    x = x[0, 0] + 0.01 * x.max()
    return (x / x.max()).contiguous()


def inputs(S, g):
    """{name: one rate plane [S, S]}"""
    import numpy as np
    import torch
    import poisson_ref as P
    planes = {f"rate_{r:g}": torch.full((S, S), float(r), device="cuda") for r in (3.0, 37.5, 1024.0)}
    planes["mixed"] = torch.from_numpy(P.mixed_rates(S * S, np.random.default_rng(7)).reshape(S, S)).cuda()
    planes["frame_32sq_photons"] = frame(S, g) * 32.0 ** 2
    return planes


def attempts_histogram(plane):
    import numpy as np
    import poisson_ref as P
    lam = plane.flatten()[:1 << 16].cpu().numpy()[None]
    _, att = P.rand_poisson(lam, SEED, return_attempts=True)
    ptrs = att[lam >= 10]
    return {"elements": int(lam.size), "inversion": int((lam < 10).sum()), "ptrs": int(ptrs.size),
            "ptrs_attempts_histogram_from_1": np.bincount(ptrs)[1:].tolist() if ptrs.size else [],
            "ptrs_attempts_mean": round(float(ptrs.mean()), 4) if ptrs.size else None,
            "ptrs_attempts_max": int(ptrs.max()) if ptrs.size else None}


def forward_problem(quick):
    import torch
    D, obj, psf = (12, 60, 216) if quick else (120, 600, 2160)
    F = obj + psf
    g = torch.Generator(device="cuda").manual_seed(2525)
    OTF = torch.view_as_complex(torch.randn(1, D, F, F // 2 + 1, 2, generator=g, device="cuda") * 1e-3)
    vol = torch.rand(1, D, obj, obj, generator=g, device="cuda")
    vol = torch.where(vol > 0.85, vol, torch.zeros((), device="cuda")) * 25
    return OTF, vol, {"depths": D, "object": obj, "psf": psf, "full": F}


def measure(quick, profile_only):
    import torch
    from cwfa_amd import ops, utils as U
    S = 216 if quick else 2160
    N = 10 if quick else 250
    g = torch.Generator(device="cuda").manual_seed(5)
    planes = inputs(S, g)
    out1, outN = torch.empty(1, S, S, device="cuda"), torch.empty(N, S, S, device="cuda")
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")
    fns, nbytes, hist = {}, {}, {}
    stacks = {}
    for name, plane in planes.items():
        one = plane[None].contiguous()
        stacks[name] = many = plane[None].expand(N, S, S).contiguous()
        hist[name] = attempts_histogram(plane)
        fns[f"rand_poisson/{name}/1"] = lambda one=one: ops.rand_poisson(one, SEED, out=out1)
        fns[f"torch.poisson/{name}/1"] = lambda one=one: torch.poisson(one)
        fns[f"rand_poisson/{name}/{N}"] = lambda many=many: ops.rand_poisson(many, SEED, out=outN)
        fns[f"torch.poisson/{name}/{N}"] = lambda many=many: torch.poisson(many)
        for k in (1, N):
            nbytes[f"rand_poisson/{name}/{k}"] = nbytes[f"torch.poisson/{name}/{k}"] = 8 * k * S * S
    fns["float4_copy"] = lambda: dst.copy_(src)
    nbytes["float4_copy"] = 8 * n_copy
    OTF, vol, shape = forward_problem(quick)
    est = torch.empty(1, 1, shape["full"], shape["full"], device="cuda")
    fns["XLFMForward"] = lambda: U.XLFMForward(OTF, vol, out=est)
    if profile_only:
        for name, f in fns.items():
            print(name, flush=True)
            f()
        torch.cuda.synchronize()
        return None
    ms = windows(fns, 3 if quick else 7, 1 if quick else 2, 1)
    res = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    copy_rate = res["float4_copy"]["GBps"]
    for k in nbytes:
        res[k]["fraction_of_measured_copy_rate"] = round(res[k]["GBps"] / copy_rate, 4)
        if k.startswith("rand_poisson/"):
            res[k]["ns_per_element"] = round(res[k]["ms"] * 1e6 / (nbytes[k] // 8), 5)
            other = res["torch.poisson/" + k.split("/", 1)[1]]
            res[k]["torch_poisson_over_rand_poisson"] = {"median": round(other["ms"] / res[k]["ms"], 3), "min": round(other["ms_min"] / res[k]["ms_max"], 3),
                                                         "max": round(other["ms_max"] / res[k]["ms_min"], 3)}
    res["XLFMForward"]["shape"] = shape
    res["attempts"] = hist
    res["config"] = {"frame": [S, S], "samples": N, "seed": SEED, "bytes_per_element": 8, "copy_elements": n_copy,
                     "frame_32sq_photons": "sparse blurred spots over a 1 % background, maximum scaled to 1024 photons"}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "poisson_time.py measures on the MI355X; there is no CPU path"
    torch.set_grad_enabled(False)
    quick, profile_only = "--quick" in sys.argv, "--profile-only" in sys.argv
    res = measure(quick, profile_only)
    if profile_only:
        return
    rec = {"workload": "shot-noise simulation: in-kernel Poisson draws, XLFM forward projection",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "poisson": res}
    out = os.path.join(ROOT, "profiles", "poisson_time_quick.json" if quick else "poisson_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("attempts", "config")}))


if __name__ == "__main__":
    main()
