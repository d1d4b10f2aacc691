#!/usr/bin/env python3
"""Time the posterior path on the MI355X and write profiles/posterior_time.json:

  * per step, at 512 x 512 with the detail-channel counts of the five halvings of a 96-plane volume (48, 24, 12, 6, 3) and a CAT step's
    five coefficient stages (channel, row, channel, column, channel gathers, composed tables): ``ops.chain_inv_var`` without and with
    a var_low plane, ``ops.chain_inv`` at z = None and with a z -- so every launch takes the 16-byte form;
  * the benchmark's pyramid (96 x 512 x 512, LRNN, split-bf16 arithmetic): 32 samples through ``posterior_samples`` against 32
    calls of ``inverse_pass``, and ``posterior_moments`` against one ``inverse_pass``.

Protocol: every shape warmed up; HIP events around windows of launches; the forms that are compared alternate inside one process;
median (min, max) over the windows.  Bytes are algorithmic (planes of C x H x W fp32 the launch must read and write), the rate is
bytes over the median time.      python tools/posterior_time.py [--quick]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fns, repeats, per_window, warmup):
    """{name: [ms per call, one per window]} for the callables of ``fns``, alternating window by window."""
    import torch
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per_window):
                f()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / per_window)
    return out


def summary(ms, nbytes=None):
    med = statistics.median(ms)
    r = {"ms": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5)}
    if nbytes:
        r["bytes_algorithmic"] = nbytes
        r["GBps"] = round(nbytes / med / 1e6, 1)
    return r


def device_record():
    import torch
    p = torch.cuda.get_device_properties(0)
    rec = {"device": p.name, "arch": getattr(p, "gcnArchName", None), "compute_units": p.multi_processor_count,
           "torch": torch.__version__, "hip": torch.version.hip, "time_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())}
    try:                                             # (needs amdsmi; absent on some boxes)
        rec["shader_clock_MHz_now"] = torch.cuda.clock_rate()
    except Exception as e:                           # noqa: BLE001
        rec["shader_clock_MHz_now"] = f"not available ({type(e).__name__})"
    try:                                             # the clocks the card reports at the time of the run (read only)
        t = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=10).stdout
        card = next(iter(json.loads(t).values()))
        rec["clocks_reported"] = {k: v for k, v in card.items() if "clk" in k.lower()}
    except Exception as e:                           # noqa: BLE001 -- the record says that the tool was not there
        rec["clocks_reported"] = f"not available ({type(e).__name__})"
    return rec


def per_step(quick):
    import torch
    from cwfa_amd import ops
    H = W = 512
    g = torch.Generator().manual_seed(3)
    res = {}
    for C_ in (48, 24, 12, 6, 3):
        axes = (1, 2, 1, 3, 1)
        perms = [torch.randperm({1: C_, 2: H, 3: W}[ax], generator=g).cuda() for ax in axes]
        st = [ops.stage(0.3 * torch.randn(1, C_, H, W, device="cuda"), torch.randn(1, C_, H, W, device="cuda"), perm=p, axis=ax)
              for p, ax in zip(perms, axes)]
        low = torch.randn(1, C_, H, W, device="cuda")
        z = torch.randn(1, C_, H, W, device="cuda")
        vl = torch.rand(1, C_, H, W, device="cuda")
        tabs = ops.chain_tables(list(zip(perms, axes)), None, C_, H, W, low.device)
        shape = (1, C_, H, W)
        fns = {"var": lambda: ops.chain_inv_var(None, st, 0.29, shape=shape, tables=tabs),
               "var_with_low": lambda: ops.chain_inv_var(vl, st, 0.29, tables=tabs),
               "inv_z_none": lambda: ops.chain_inv(None, low, st, tables=tabs),
               "inv_with_z": lambda: ops.chain_inv(z, low, st, tables=tabs)}
        plane = 4 * C_ * H * W
        planes = {"var": 5 + 2, "var_with_low": 5 + 1 + 2, "inv_z_none": 10 + 1 + 2, "inv_with_z": 10 + 2 + 2}     # s (, t) rows + inputs + the output pair
        ms = windows(fns, 3 if quick else 15, 5 if quick else 200, 3)
        res[f"C{C_}"] = {k: dict(summary(v, planes[k] * plane), planes=planes[k]) for k, v in ms.items()}
        assert torch.equal(fns["var"](), fns["var"]())
    return res


def pyramid(quick):
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
        N = 4 if quick else 32

        def recon():
            with torch.no_grad():
                return CWFA.inverse_pass(conv_inn, cond_nets, cond_input, mean_cache, low=low)

        def recon_n():
            for _ in range(N):
                recon()

        fns = {"inverse_pass": recon,
               "posterior_moments": lambda: CWFA.posterior_moments(conv_inn, cond_nets, cond_input, mean_cache, low=low, temperature=1.0),
               f"inverse_pass_x{N}": recon_n,
               f"posterior_samples_{N}": lambda: CWFA.posterior_samples(conv_inn, cond_nets, cond_input, mean_cache, N, low=low, temperature=1.0)}
        ms = windows(fns, 3 if quick else 7, 1 if quick else 3, 2)
        res = {k: summary(v) for k, v in ms.items()}
        res["moments_over_inverse_pass"] = round(res["posterior_moments"]["ms"] / res["inverse_pass"]["ms"], 4)
        res["samples_speedup_vs_inverse_passes"] = round(res[f"inverse_pass_x{N}"]["ms"] / res[f"posterior_samples_{N}"]["ms"], 2)
        res["ms_per_sample"] = round(res[f"posterior_samples_{N}"]["ms"] / N, 4)
        res["config"] = {"depths": D, "side": side, "flow_steps": S - 1, "lrnn": not quick, "precision": "split_bf16", "batch": 1, "samples": N,
                         "note": "inverse_pass in train-mode LRNN (dropout draws differ between calls); posterior_samples includes the latent draws"}
        return res
    finally:
        ops.set_precision("fp32")


def main():
    import torch
    assert torch.cuda.is_available(), "posterior_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "posterior of a CAT pyramid: closed-form variance launch, shared-coefficient samples",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, compared forms alternating in one process",
           "box": device_record(), "per_step_512x512": per_step(quick), "pyramid": pyramid(quick)}
    out = os.path.join(ROOT, "profiles", "posterior_time_quick.json" if quick else "posterior_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["pyramid"]))
    print(json.dumps({k: {n: (v["ms"], v.get("GBps")) for n, v in r.items()} for k, r in rec["per_step_512x512"].items()}))


if __name__ == "__main__":
    main()
