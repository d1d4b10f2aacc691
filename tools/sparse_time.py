#!/usr/bin/env python3
"""Time sparse-activity extraction on the MI355X and write profiles/sparse_time.json.

At 250 x 2160 x 2160 (the reference's raw stack: 4.7 GB fp32, 2.3 GB fp16), one GPU process, for fp32 and fp16:

  * ``ops.temporal_select`` in the one-read form and in the streaming form (the median), and with a background and two ranks
    (pass B of ``extract_sparse``);
  * ``ops.frame_dots``, ``ops.sparse_residual`` (map and pair layout);
  * the whole ``extract_sparse`` without and with pass B;
  * the same pipeline in torch operators on the same card: ``torch.kthvalue`` along dim 0, a matrix-vector product, elementwise;
  * a float4 copy of 1 GiB (``Tensor.copy_``): the yardstick.  The select kernel is held against the time to read the stack once at
    that copy rate; the ratio is recorded.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.
    python tools/sparse_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402


def torch_pipeline(x, rank):
    """extract_sparse(noise_k=0) in torch operators: a k-th value along time, a matrix-vector product, elementwise."""
    import torch
    T = x.shape[0]
    b = torch.kthvalue(x, rank + 1, dim=0).values
    flat, bf = x.reshape(T, -1), b.reshape(-1)
    a = ((flat @ bf).float() / (bf.float() @ bf.float())).to(x.dtype)
    return torch.relu(x - a[:, None, None] * b), b


def measure(quick):
    import torch
    from cwfa_amd import ops
    from cwfa_amd.XLFMDataset import extract_sparse, quantile_rank
    T, H, W = (60, 256, 256) if quick else (250, 2160, 2160)
    P = H * W
    g = torch.Generator(device="cuda").manual_seed(5)
    x32 = torch.empty(T, H, W, device="cuda")
    for t in range(T):                                             # counts of a few hundred with noise, frame by frame: no 2nd stack
        x32[t] = torch.floor(300.0 + 200.0 * torch.rand(H, W, device="cuda", generator=g) - 0.3 * t)
    stacks = {"fp32": x32, "fp16": x32.half()}
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")
    rank = quantile_rank(0.5, T)
    ranks_b = [quantile_rank(0.5, T), quantile_rank(0.1587, T)]
    fast, slow, nbytes, checks = {"float4_copy": lambda: dst.copy_(src)}, {}, {"float4_copy": 8 * n_copy}, {}
    for name, x in stacks.items():
        es = x.element_size()
        base = ops.temporal_select(x, [rank])[0]
        a = torch.linspace(1.1, 0.9, T, device="cuda")
        tau = torch.full_like(base, 3.0)
        fast[f"select_lds_{name}"] = lambda x=x: ops.temporal_select(x, [rank], form="lds")
        slow[f"select_stream_{name}"] = lambda x=x: ops.temporal_select(x, [rank], form="stream")
        fast[f"select_lds_background_2ranks_{name}"] = lambda x=x, a=a, base=base: ops.temporal_select(x, ranks_b, a=a, b=base, form="lds")
        fast[f"frame_dots_{name}"] = lambda x=x, base=base: ops.frame_dots(x, base)
        fast[f"residual_{name}"] = lambda x=x, a=a, base=base, tau=tau: ops.sparse_residual(x, a, base, tau)
        fast[f"residual_pair_{name}"] = lambda x=x, a=a, base=base, tau=tau: ops.sparse_residual(x, a, base, tau, pair=True)
        fast[f"extract_sparse_{name}"] = lambda x=x: extract_sparse(x)
        fast[f"extract_sparse_noise_k3_{name}"] = lambda x=x: extract_sparse(x, noise_k=3.0)
        slow[f"torch_pipeline_{name}"] = lambda x=x: torch_pipeline(x, rank)
        stack = T * P * es
        nbytes.update({f"select_lds_{name}": stack + 4 * P, f"select_stream_{name}": stack + 4 * P,
                       f"select_lds_background_2ranks_{name}": stack + 12 * P, f"frame_dots_{name}": stack + 4 * P,
                       f"residual_{name}": stack + 4 * T * P + 8 * P, f"residual_pair_{name}": stack + 8 * T * P + 8 * P,
                       f"extract_sparse_{name}": 3 * stack + 4 * T * P + 12 * P,
                       f"extract_sparse_noise_k3_{name}": 4 * stack + 4 * T * P + 28 * P})
        checks[f"forms_agree_{name}"] = bool(torch.equal(ops.temporal_select(x, [rank], form="stream")[0], base))
        checks[f"kthvalue_agrees_{name}"] = bool(torch.equal(torch.kthvalue(x, rank + 1, dim=0).values.float(), base))
        del base
    ms = windows(fast, 3 if quick else 5, 1 if quick else 2, 1)
    ms.update(windows(slow, 2 if quick else 3, 1, 1))
    res = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    copy_rate = res["float4_copy"]["GBps"]
    for k in nbytes:
        res[k]["fraction_of_measured_copy_rate"] = round(res[k]["GBps"] / copy_rate, 3)
    for name, x in stacks.items():
        read_once_ms = T * P * x.element_size() / copy_rate / 1e6
        res[f"select_lds_{name}"]["stack_read_once_at_copy_rate_ms"] = round(read_once_ms, 4)
        res[f"select_lds_{name}"]["time_over_one_read_at_copy_rate"] = round(res[f"select_lds_{name}"]["ms"] / read_once_ms, 2)
        res[f"select_stream_{name}"]["time_over_one_read_at_copy_rate"] = round(res[f"select_stream_{name}"]["ms"] / read_once_ms, 2)
        res[f"stream_over_lds_{name}"] = round(res[f"select_stream_{name}"]["ms"] / res[f"select_lds_{name}"]["ms"], 2)
        res[f"torch_pipeline_over_extract_sparse_{name}"] = round(res[f"torch_pipeline_{name}"]["ms"] / res[f"extract_sparse_{name}"]["ms"], 2)
    res["checks"] = checks
    res["config"] = {"stack": [T, H, W], "rank": rank, "ranks_pass_b": ranks_b, "copy_elements": n_copy,
                     "lds_frames": {"fp32": ops.temporal_lds_frames(torch.float32), "fp16": ops.temporal_lds_frames(torch.float16),
                                    "background": ops.temporal_lds_frames(torch.float16, True)}}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "sparse_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "sparse-activity extraction: temporal selection, frame dots, residual, extract_sparse",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "sparse": measure(quick)}
    out = os.path.join(ROOT, "profiles", "sparse_time_quick.json" if quick else "sparse_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["sparse"]))


if __name__ == "__main__":
    main()
