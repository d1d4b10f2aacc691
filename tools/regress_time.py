#!/usr/bin/env python3
"""Time the streaming regression maps on the MI355X and write profiles/regress_time.json.

At 96 x 512 x 512 (the benchmark's volume), one GPU process, for K = 1, 4, 8, 16 regressors:

  * ``RegressionMap.update`` (the update launch or launches and the launch of the regressors' own sums) per volume, fed in chunks of
    16 and one volume at a time;
  * beside it, measured in the same run: ``ActivityMap.update`` fed the same way; the update's byte floor -- the chunk read, the
    state of 28 + 8 K bytes per voxel read and written (x0 is not written after the first chunk; with K > 8 the chunk and x0 are
    read twice), at the rate of a float4 copy of 1 GiB -- and the torch-operator form of the sums p, a float64 ``einsum`` over a
    resident float64 slab of 16 volumes (which the streaming form exists to avoid);
  * ``RegressionMap.finish`` per output set: corr alone, t alone, all four.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.
    python tools/regress_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402

KS = (1, 4, 8, 16)
SETS = {"corr": ("corr",), "t": ("t",), "all": ("corr", "beta", "t", "r2")}


def update_bytes(m, K, chunk):
    """What one update call of ``chunk`` volumes has to move, by the kernels' own accesses (not the first chunk)."""
    passes = 2 if K > 8 else 1
    return (4 * chunk * passes + 4 * passes + 24 + 24 + 16 * K) * m


def measure(quick):
    import torch
    from cwfa_amd import CWFA
    D, H, W = (24, 128, 128) if quick else (96, 512, 512)
    m, chunk = D * H * W, 16
    g = torch.Generator(device="cuda").manual_seed(5)
    vols = 100.0 + torch.randn(chunk, D, H, W, device="cuda", generator=g)
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")
    am = CWFA.ActivityMap((D, H, W), "cuda").update(vols)

    def one_by_one(obj, *rows):
        for t in range(chunk):
            obj.update(vols[t], *(r[t] for r in rows))

    res = {}
    base = {"activity_update_chunks_of_16": lambda: am.update(vols), "activity_update_chunks_of_1": lambda: one_by_one(am),
            "float4_copy": lambda: dst.copy_(src)}
    reps = (3, 1, 1) if quick else (7, 2, 2)
    for K in KS:
        # four chunks of distinct rows first: 16 regressors and the intercept need more than 16 distinct rows to be fitted
        pool = torch.randn(4 * chunk, K, dtype=torch.float64, device="cuda", generator=g)
        rm = CWFA.RegressionMap((D, H, W), "cuda", K)
        for c in range(4):
            rm.update(vols, pool[c * chunk:(c + 1) * chunk])
        rows = pool[:chunk]
        slab = vols.double().sub_(vols[0].double()).view(chunk, m)
        fns = dict(base)
        fns["update_chunks_of_16"] = lambda: rm.update(vols, rows)
        fns["update_chunks_of_1"] = lambda: one_by_one(rm, rows)
        fns["torch_einsum_resident_f64"] = lambda: torch.einsum("tk,tv->kv", rows, slab)
        for name, want in SETS.items():
            fns["finish_" + name] = lambda want=want: rm.finish(want=want)
        ms = windows(fns, *reps)
        nbytes = {"update_chunks_of_16": update_bytes(m, K, chunk), "update_chunks_of_1": chunk * update_bytes(m, K, 1),
                  "activity_update_chunks_of_16": (4 * chunk + 28 + 24) * m, "activity_update_chunks_of_1": chunk * (4 + 28 + 24) * m,
                  "float4_copy": 8 * n_copy, "torch_einsum_resident_f64": (8 * chunk + 8 * K) * m}
        r = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
        copy_rate = r["float4_copy"]["GBps"]
        for k in ("update_chunks_of_16", "update_chunks_of_1", "activity_update_chunks_of_16", "activity_update_chunks_of_1",
                  "torch_einsum_resident_f64"):
            r[k]["ms_per_volume"] = round(r[k]["ms"] / chunk, 5)
        for k in ("update_chunks_of_16", "update_chunks_of_1"):
            r[k]["byte_floor_ms_per_volume_at_measured_copy_rate"] = round(nbytes[k] / copy_rate / 1e6 / chunk, 5)
            r[k]["fraction_of_measured_copy_rate"] = round(r[k]["GBps"] / copy_rate, 3)
            r[k]["over_plain_activity_update"] = round(r[k]["ms"] / r["activity_" + k]["ms"], 3)
            # 2 K + 3 float64 operations and 2 conversions per voxel and sample, as the kernel performs them
            r[k]["f64_Gops_per_s"] = round((2 * K + 5) * m * chunk / r[k]["ms"] / 1e6, 1)
        r["state_bytes"] = (28 + 8 * K) * m
        res[f"K={K}"] = r
        del rm, slab, rows
        torch.cuda.empty_cache()
    res["config"] = {"volume": [D, H, W], "chunk": chunk, "copy_elements": n_copy, "regressors": list(KS),
                     "series": "100 + standard normal", "einsum_slab_volumes": chunk}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "regress_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "regression maps: streaming per-voxel GLM update, design, per-voxel finish",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "regress": measure(quick)}
    out = os.path.join(ROOT, "profiles", "regress_time_quick.json" if quick else "regress_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["regress"]))


if __name__ == "__main__":
    main()
