#!/usr/bin/env python3
"""Time neuron detection on the MI355X and write profiles/neuron_time.json.

At 96 x 512 x 512 (the benchmark's volume), one GPU process:

  * ``ActivityMap.update`` per volume, fed one volume at a time and in chunks of 16;
  * ``ActivityMap.finish``;
  * ``ops.local_maxima`` at the workload's half-widths (5, 9, 9), device work and the read-back of the peaks;
  * the torch-operator form of the detector on the same card: ``F.max_pool3d`` over the 11 x 19 x 19 window, ``==``, the threshold,
    ``nonzero``, ``topk``;
  * a float4 copy of 1 GiB (``Tensor.copy_``), the yardstick for what a streaming kernel can reach from HBM.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.  Each record carries the bytes the kernels have to move and the fraction of the copy rate that is: of the yardstick measured
in the same run, and of the 6.29 TB/s the project quotes for it.
    python tools/neuron_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402

COPY_TBPS_QUOTED = 6.29


def measure(quick):
    import torch
    import torch.nn.functional as F
    from cwfa_amd import CWFA, _lib, ops
    D, H, W = (24, 128, 128) if quick else (96, 512, 512)
    m = D * H * W
    dist, thr, chunk = (5, 9, 9), 0.5, 16
    g = torch.Generator(device="cuda").manual_seed(5)
    vols = torch.rand(chunk, D, H, W, device="cuda", generator=g)
    score = torch.rand(D, H, W, device="cuda", generator=g)
    am = CWFA.ActivityMap((D, H, W), "cuda").update(vols)
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")

    def one_by_one():
        for t in range(chunk):
            am.update(vols[t])

    kernel = (2 * dist[0] + 1, 2 * dist[1] + 1, 2 * dist[2] + 1)

    def torch_form():
        top = F.max_pool3d(score[None, None], kernel, 1, dist)[0, 0]
        idx = ((score == top) & (score >= thr)).nonzero()
        vals = score[idx[:, 0], idx[:, 1], idx[:, 2]]
        order = torch.topk(vals, vals.numel()).indices
        return idx[order].cpu(), vals[order].cpu()

    # the two launches alone, on buffers allocated once: no read-back, no host sort
    L = _lib.lib()
    ws = torch.empty(m, dtype=torch.int64, device="cuda")
    out = torch.empty(1 << 20, 2, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")

    def launches():
        _lib.check(L.cwfa_local_maxima_f32(ops._p(score), D, H, W, thr, *dist, 0, 0, 0, ops._p(ws), ops._p(out), out.shape[0], ops._p(count),
                                           ops._stream()), "local_maxima")

    fns = {"update_chunks_of_1": one_by_one, "update_chunks_of_16": lambda: am.update(vols), "finish": lambda: am.finish("std"),
           "local_maxima": lambda: ops.local_maxima(score, thr, dist), "local_maxima_launches_only": launches,
           "torch_operator_form": torch_form, "float4_copy": lambda: dst.copy_(src)}
    ms = windows(fns, 3 if quick else 7, 1 if quick else 2, 1 if quick else 2)
    # bytes each form has to move.  update: the chunk in, 28 bytes of state in, 24 out (x0 is written by the first chunk only);
    # finish: the state in, three maps out; local_maxima: the map in and the 64-bit in-plane maxima out, then those in again
    nbytes = {"update_chunks_of_1": chunk * (4 + 28 + 24) * m, "update_chunks_of_16": (4 * chunk + 28 + 24) * m, "finish": (28 + 12) * m,
              "local_maxima": (4 + 8 + 8) * m, "local_maxima_launches_only": (4 + 8 + 8) * m, "float4_copy": 8 * n_copy}
    res = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    copy_rate = res["float4_copy"]["GBps"]
    for k in nbytes:
        res[k]["fraction_of_measured_copy_rate"] = round(res[k]["GBps"] / copy_rate, 3)
        res[k]["fraction_of_quoted_copy_rate"] = round(res[k]["GBps"] / (COPY_TBPS_QUOTED * 1e3), 3)
    for k in ("update_chunks_of_1", "update_chunks_of_16"):
        res[k]["ms_per_volume"] = round(res[k]["ms"] / chunk, 5)
    zyx, sc, total = ops.local_maxima(score, thr, dist)
    t_idx, t_val = torch_form()
    res["local_maxima"]["peaks"] = total
    res["local_maxima"]["includes"] = "both launches, the read-back of the counter and of the peaks, the host sort"
    res["torch_operator_form"]["peaks"] = int(t_idx.shape[0])
    res["torch_operator_form"]["same_peak_set"] = bool(sorted(map(tuple, zyx.tolist())) == sorted(map(tuple, t_idx.tolist())))
    res["local_maxima_over_torch_form"] = {"median": round(res["torch_operator_form"]["ms"] / res["local_maxima"]["ms"], 2),
                                           "min": round(res["torch_operator_form"]["ms_min"] / res["local_maxima"]["ms_max"], 2),
                                           "max": round(res["torch_operator_form"]["ms_max"] / res["local_maxima"]["ms_min"], 2)}
    res["config"] = {"volume": [D, H, W], "dist": list(dist), "thr": thr, "chunk": chunk, "map": "uniform random (no ties)",
                     "copy_elements": n_copy, "state_bytes": 28 * m}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "neuron_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "neuron detection: streaming activity map, 3-D local maxima",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "neurons": measure(quick)}
    out = os.path.join(ROOT, "profiles", "neuron_time_quick.json" if quick else "neuron_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["neurons"]))


if __name__ == "__main__":
    main()
