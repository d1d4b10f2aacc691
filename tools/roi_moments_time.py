#!/usr/bin/env python3
"""Time the exact ROI-mean moments on the MI355X and write profiles/roi_moments_time.json.

The benchmark's pyramid (96 x 512 x 512, four flow steps plus the LRNN, split-bf16 arithmetic, batch 1), one frame per call:

  * ``posterior_moments``                                   the per-voxel route the new call is built beside;
  * ``posterior_roi_moments`` with 13 boxes                 (r12 = 4, r3 = 2: the boxes of tools/posterior_sampler_time.py);
  * ``posterior_roi_moments`` with 4096 boxes               (r12 = 5, r3 = 3, seeded random centres);
  * ``posterior_roi_means`` with 256 samples and 13 boxes   the sampling route to the same error bar;

and, for the choice of the box transport, both ROI forms again with the other transport forced: the boxes in the kernel arguments
(64 pairs per launch) against one device table (one upload per call, one launch per step).

Protocol of tools/posterior_sampler_time.py: every form warmed up; HIP events around windows of calls; the compared forms alternate
inside one process; median (min, max) over the windows; the box's identity in the record.
    python tools/roi_moments_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402


def pyramid(quick):
    import numpy as np
    import torch
    from cwfa_amd import CWFA, ops
    torch.manual_seed(0)
    side, D, S = (128, 32, 3) if quick else (512, 96, 5)
    ops.set_precision("split_bf16")
    default_switch = ops.ROI_COV_ARG_PAIRS
    try:
        conv_inn, cond_nets = CWFA.build_networks(D, side, S, with_lrnn=not quick, device="cuda")
        g = torch.Generator().manual_seed(1)
        cond_input = torch.randn(1, 29, side, side, generator=g).cuda()
        mean_cache = [(0.1 * torch.randn(1, D // 2 ** (n + 1), side, side, generator=g)).cuda() for n in range(S - 1)]
        low = torch.randn(1, D // 2 ** (S - 1), side, side, generator=g).cuda() if quick else None
        NR, NB = (8, 256) if quick else (256, 4096)
        rs = np.random.RandomState(2)
        coords = [(int(rs.randint(8, side - 8)), int(rs.randint(8, side - 8)), int(rs.randint(-10, 10))) for _ in range(13)]
        boxes13 = CWFA.roi_boxes(coords, (1, D, side, side), 4, 2)
        many = [(int(rs.randint(0, side)), int(rs.randint(0, side)), int(rs.randint(-D // 2 + 16, D // 2 + 10))) for _ in range(NB)]    # every box inside
        boxes_many = CWFA.roi_boxes(many, (1, D, side, side), 5, 3)
        args = (conv_inn, cond_nets, cond_input, mean_cache)

        def forced(boxes, switch):
            def run():
                ops.ROI_COV_ARG_PAIRS = switch
                try:
                    return CWFA.posterior_roi_moments(*args, boxes, low=low, temperature=1.0)
                finally:
                    ops.ROI_COV_ARG_PAIRS = default_switch
            return run

        ARGS, TABLE = 1 << 30, 0
        fns = {"posterior_moments": lambda: CWFA.posterior_moments(*args, low=low, temperature=1.0),
               "posterior_roi_moments_13_boxes": lambda: CWFA.posterior_roi_moments(*args, boxes13, low=low, temperature=1.0),
               f"posterior_roi_moments_{NB}_boxes": lambda: CWFA.posterior_roi_moments(*args, boxes_many, low=low, temperature=1.0),
               "roi_moments_13_boxes_kernel_arguments": forced(boxes13, ARGS),
               "roi_moments_13_boxes_device_table": forced(boxes13, TABLE),
               f"roi_moments_{NB}_boxes_kernel_arguments": forced(boxes_many, ARGS),
               f"roi_moments_{NB}_boxes_device_table": forced(boxes_many, TABLE)}
        ms = windows(fns, 3 if quick else 7, 1 if quick else 3, 2)
        res = {k: summary(v) for k, v in ms.items()}
        roi = windows({"roi": lambda: CWFA.posterior_roi_means(*args, boxes13, NR, low=low, temperature=1.0, seed=7, chunk=16)},
                      3 if quick else 5, 1, 1)
        sampled = summary(roi["roi"])
        res[f"posterior_roi_means_{NR}_samples_13_boxes"] = dict(sampled, note="ms per frame: networks once, 16 samples per chunk")
        base = res["posterior_moments"]
        for name in ("posterior_roi_moments_13_boxes", f"posterior_roi_moments_{NB}_boxes"):
            r = res[name]
            r["overhead_over_posterior_moments_ms"] = {"median": round(r["ms"] - base["ms"], 4), "min": round(r["ms_min"] - base["ms_max"], 4),
                                                       "max": round(r["ms_max"] - base["ms_min"], 4)}
            r["sampled_route_over_this"] = {"median": round(sampled["ms"] / r["ms"], 3), "min": round(sampled["ms_min"] / r["ms_max"], 3),
                                            "max": round(sampled["ms_max"] / r["ms_min"], 3)}
        # the two transports agree bit for bit (behind a given coarsest volume: the train-mode LRNN is not part of the comparison)
        fixed = torch.randn(1, D // 2 ** (S - 1), side, side, generator=g).cuda()
        both = []
        for switch in (ARGS, TABLE):
            ops.ROI_COV_ARG_PAIRS = switch
            both.append(CWFA.posterior_roi_moments(*args, boxes_many, low=fixed, temperature=1.0))
        ops.ROI_COV_ARG_PAIRS = default_switch
        (m_a, s_a, _), (m_b, s_b, _) = both
        res["transports_bitwise_equal"] = bool(torch.equal(m_a, m_b) and torch.equal(s_a, s_b))
        res["std_over_abs_mean_median"] = round(float((s_a / m_a.abs()).median()), 4)
        assert res["transports_bitwise_equal"] and bool((s_a > 0).all()), (res["transports_bitwise_equal"], int((~(s_a > 0)).sum()))
        res["config"] = {"depths": D, "side": side, "flow_steps": S - 1, "lrnn": not quick, "precision": "split_bf16", "batch": 1,
                         "samples_of_the_sampled_route": NR, "boxes_many": NB, "pairs_per_launch_in_kernel_arguments": default_switch,
                         "note": "every form runs every network once per call (train-mode LRNN included)"}
        return res
    finally:
        ops.ROI_COV_ARG_PAIRS = default_switch
        ops.set_precision("fp32")


def main():
    import torch
    assert torch.cuda.is_available(), "roi_moments_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "exact ROI-mean posterior moments: posterior_moments' loop with one ROI covariance launch per step",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, compared forms alternating in one process",
           "box": device_record(), "pyramid": pyramid(quick)}
    out = os.path.join(ROOT, "profiles", "roi_moments_time_quick.json" if quick else "roi_moments_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["pyramid"]))


if __name__ == "__main__":
    main()
