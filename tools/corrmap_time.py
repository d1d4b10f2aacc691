#!/usr/bin/env python3
"""Time the streaming local-correlation map on the MI355X and write profiles/corrmap_time.json.

At 96 x 512 x 512 (the benchmark's volume), one GPU process:

  * the plain ``ActivityMap.update`` in a chunk of 16: the reference point, section 22's kernel;
  * ``ActivityMap(neighbours=6 / 8 / 26).update`` in a chunk of 16 and fed one volume at a time;
  * ``ops.correlation_finish`` at each;
  * the torch-operator form a user would otherwise write, on a resident stack of 16: standardise the series, multiply it with
    itself shifted by each forward offset, take the mean over time, add to both voxels of the pair, divide by the neighbour count;
  * a float4 copy of 1 GiB (``Tensor.copy_``), the yardstick for what a streaming kernel can reach from HBM.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.  Each record carries the byte floor of the form -- per voxel and call 4 T' for the chunk, once, and 2 (28 + 8 K) for the
state in and out; the finish reads 16 + 8 K and writes 4 -- the time that floor takes at the copy rate measured in the same run,
and the form's time as a multiple of it, of the plain update and of the torch form.
    python tools/corrmap_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402

FORWARD = {6: [(0, 0, 1), (0, 1, 0), (1, 0, 0)],
           8: [(0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1)],
           26: [(0, 0, 1)] + [(0, 1, dx) for dx in (-1, 0, 1)] + [(1, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]}


def pair(shape, o):
    """Slices (lo, hi) of a [.., D, H, W] tensor: the voxels whose neighbour at offset o is inside the volume, and those neighbours."""
    lo = tuple(slice(max(0, -d), n - max(0, d)) for n, d in zip(shape, o))
    hi = tuple(slice(max(0, d), n - max(0, -d)) for n, d in zip(shape, o))
    return (Ellipsis, *lo), (Ellipsis, *hi)


def measure(quick):
    import torch
    from cwfa_amd import CWFA, ops
    D, H, W = (24, 128, 128) if quick else (96, 512, 512)
    shape, m, chunk = (D, H, W), D * H * W, 16
    g = torch.Generator(device="cuda").manual_seed(5)
    vols = torch.rand(chunk, D, H, W, device="cuda", generator=g)
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")
    plain = CWFA.ActivityMap(shape, "cuda").update(vols)
    maps = {nb: CWFA.ActivityMap(shape, "cuda", neighbours=nb).update(vols) for nb in FORWARD}

    def one_by_one(am):
        for t in range(chunk):
            am.update(vols[t])

    def torch_form(nb):
        z = (vols - vols.mean(0)) / vols.std(0, unbiased=False)
        total, n = torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda")
        for o in FORWARD[nb]:
            lo, hi = pair(shape, o)
            r = (z[lo] * z[hi]).mean(0)
            total[lo[1:]] += r
            total[hi[1:]] += r
            n[lo[1:]] += 1
            n[hi[1:]] += 1
        return total / n

    fns = {"plain_update_chunk_of_16": lambda: plain.update(vols), "float4_copy": lambda: dst.copy_(src)}
    nbytes = {"plain_update_chunk_of_16": (4 * chunk + 28 + 24) * m, "float4_copy": 8 * n_copy}
    for nb, am in maps.items():
        K = len(FORWARD[nb])
        fns[f"corr{nb}_update_chunk_of_16"] = lambda am=am: am.update(vols)
        fns[f"corr{nb}_update_chunks_of_1"] = lambda am=am: one_by_one(am)
        fns[f"corr{nb}_finish"] = lambda am=am, nb=nb: ops.correlation_finish(am.state, am.cc, am.count, nb)
        fns[f"torch{nb}_operator_form"] = lambda nb=nb: torch_form(nb)
        nbytes[f"corr{nb}_update_chunk_of_16"] = (4 * chunk + 2 * (28 + 8 * K)) * m
        nbytes[f"corr{nb}_update_chunks_of_1"] = chunk * (4 + 2 * (28 + 8 * K)) * m
        nbytes[f"corr{nb}_finish"] = (16 + 8 * K + 4) * m
    ms = windows(fns, 3 if quick else 7, 1 if quick else 2, 1 if quick else 2)
    res = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    copy_rate = res["float4_copy"]["GBps"]
    base = res["plain_update_chunk_of_16"]["ms"]
    for k in nbytes:
        res[k]["floor_ms_at_measured_copy_rate"] = round(nbytes[k] / copy_rate / 1e6, 5)
        res[k]["multiple_of_floor"] = round(res[k]["ms"] / res[k]["floor_ms_at_measured_copy_rate"], 2)
    for nb in FORWARD:
        tf = res[f"torch{nb}_operator_form"]
        for form in ("update_chunk_of_16", "update_chunks_of_1"):
            r = res[f"corr{nb}_{form}"]
            r["ms_per_volume"] = round(r["ms"] / chunk, 5)
            r["multiple_of_plain_update_chunk_of_16"] = round(r["ms"] / base, 2)
        both = res[f"corr{nb}_update_chunk_of_16"]["ms"] + res[f"corr{nb}_finish"]["ms"]
        tf["over_update_chunk_of_16_plus_finish"] = {"median": round(tf["ms"] / both, 2)}
        # the two forms compute the same map up to fp32 rounding of the torch one: the largest difference, for the record
        fresh = CWFA.ActivityMap(shape, "cuda", neighbours=nb).update(vols)
        tf["max_abs_difference_from_the_streamed_map"] = float((fresh.finish("corr")[0] - torch_form(nb)).abs().max())
    res["config"] = {"volume": [D, H, W], "chunk": chunk, "volumes": "uniform random", "copy_elements": n_copy,
                     "state_bytes": {str(nb): (28 + 8 * len(FORWARD[nb])) * m for nb in FORWARD}}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "corrmap_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "streaming local-correlation map: update with pair sums, finish, the torch-operator form",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "corrmap": measure(quick)}
    out = os.path.join(ROOT, "profiles", "corrmap_time_quick.json" if quick else "corrmap_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["corrmap"]))


if __name__ == "__main__":
    main()
