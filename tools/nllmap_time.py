#!/usr/bin/env python3
"""Time the likelihood maps on the MI355X and write profiles/nllmap_time.json:

  * per step, at 512 x 512 with 48 / 24 / 12 / 6 detail channels and a CAT step's five coefficient stages (channel, row, channel,
    column, channel gathers, composed tables): one ``ops.chain_nll_map`` launch (nll + low + the per-sample sum; the same with the
    z-scores; the general form on an x that is one float off the 16-byte grid) beside ``ops.chain_fwd`` with ``logdet`` and ``sumsq``
    on the same stages, and the ``ops.nll_compose`` of those levels;
  * the benchmark's pyramid (96 x 512 x 512, LRNN, split-bf16 arithmetic): ``CWFA.nll_maps`` (with and without the z-scores) beside
    ``CWFA.forward_nll_pass``.

Protocol of tools/posterior_time.py: every form warmed up; HIP events around windows of calls; the compared forms alternate inside one
process; median (min, max) over the windows; the box's identity in the record.  Bytes are algorithmic: per step 14 C planes (the
pair in, ten coefficient rows, nll and low out), 15 with the z-scores.      python tools/nllmap_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402


def per_step(quick):
    import torch
    from cwfa_amd import ops
    H = W = 128 if quick else 512
    g = torch.Generator().manual_seed(3)
    res, levels = {}, []
    for C_ in (48, 24, 12, 6):
        axes = (1, 2, 1, 3, 1)
        perms = [torch.randperm({1: C_, 2: H, 3: W}[ax], generator=g).cuda() for ax in axes]
        st = [ops.stage(0.3 * torch.randn(1, C_, H, W, device="cuda"), torch.randn(1, C_, H, W, device="cuda"), perm=p, axis=ax)
              for p, ax in zip(perms, axes)]
        x = torch.randn(1, 2 * C_, H, W, device="cuda")
        buf = torch.empty(x.numel() + 4, device="cuda")
        x_off = buf[1:1 + x.numel()].view(x.shape)
        x_off.copy_(x)
        tabs = ops.chain_tables(list(zip(perms, axes)), None, C_, H, W, x.device)
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        ld, sq = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
        fns = {"nll_map": lambda: ops.chain_nll_map(x, st, tables=tabs, nll_sum=acc),
               "chain_fwd_logdet_sumsq": lambda: ops.chain_fwd(x, st, logdet=ld, sumsq=sq, tables=tabs),
               "nll_map_with_z": lambda: ops.chain_nll_map(x, st, tables=tabs, want_z=True, nll_sum=acc),
               "nll_map_general_form": lambda: ops.chain_nll_map(x_off, st, nll_sum=acc)}
        plane = 4 * C_ * H * W
        planes = {"nll_map": 14, "chain_fwd_logdet_sumsq": 14, "nll_map_with_z": 15, "nll_map_general_form": 14}
        ms = windows(fns, 3 if quick else 9, 2 if quick else 20, 3)
        r = {k: summary(v, planes[k] * plane) for k, v in ms.items()}
        r["ratio_nll_map_to_chain_fwd"] = round(r["nll_map"]["ms"] / r["chain_fwd_logdet_sumsq"]["ms"], 3)
        res[f"C{C_}"] = r
        a, b = fns["nll_map"](), fns["nll_map"]()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        levels.append(a[0])
        del st, x, x_off, buf
        torch.cuda.empty_cache()
    ms = windows({"nll_compose": lambda: ops.nll_compose(levels)}, 3 if quick else 9, 2 if quick else 20, 3)
    nbytes = 4 * H * W * (96 + sum(lv.shape[1] for lv in levels))
    res["compose_4_levels_96_depths"] = summary(ms["nll_compose"], nbytes)
    res["sizes"] = {"H": H, "W": W, "stages": 5}
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
        vol = torch.randn(1, D, side, side, generator=g).cuda()
        args = (conv_inn, cond_nets, vol, cond_input, mean_cache)

        def fwd():
            with torch.no_grad():
                return CWFA.forward_nll_pass(*args)
        fns = {"nll_maps": lambda: CWFA.nll_maps(*args), "forward_nll_pass": fwd, "nll_maps_with_z": lambda: CWFA.nll_maps(*args, want_z=True)}
        ms = windows(fns, 3 if quick else 7, 1 if quick else 3, 2)
        res = {k: summary(v) for k, v in ms.items()}
        res["ratio_nll_maps_to_forward_nll_pass"] = round(res["nll_maps"]["ms"] / res["forward_nll_pass"]["ms"], 3)
        res["config"] = {"depths": D, "side": side, "flow_steps": S - 1, "lrnn": not quick, "precision": "split_bf16", "batch": 1,
                         "note": "both run every condition net and sub-network once per step; nll_maps adds one compose launch"}
        return res
    finally:
        ops.set_precision("fp32")


def main():
    import torch
    assert torch.cuda.is_available(), "nllmap_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "per-voxel likelihood maps and z-scores of a CAT pyramid: one launch per step + one compose",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, compared forms alternating in one process",
           "box": device_record(), "per_step": per_step(quick), "pyramid": pyramid(quick)}
    out = os.path.join(ROOT, "profiles", "nllmap_time_quick.json" if quick else "nllmap_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["pyramid"]))
    print(json.dumps({k: {n: (v["ms"], v.get("GBps")) for n, v in r.items() if isinstance(v, dict)} for k, r in rec["per_step"].items() if k != "sizes"}))


if __name__ == "__main__":
    main()
