#!/usr/bin/env python3
"""Time per-lenslet frame registration on the MI355X and write profiles/register_views_time.json.

At 250 x 2160 x 2160 with 29 lenslet views of 512 x 512 (the view size of the reference's main.py: ``--volume_side_size``), the
centres on a hexagonal lattice of 380 px around the middle of the sensor (neighbouring boxes overlap, as they do on the instrument),
one GPU process, for fp32 and fp16:

  * ``ops.reg_window_views`` on one chunk of frames, against its own bytes at the copy rate;
  * the transforms of that chunk (``torch.fft.rfft2`` / ``irfft2``), ``ops.reg_whiten`` and ``ops.reg_peak`` on its batch of views;
  * ``ops.reg_fit_views`` for the whole stack, ``ops.reg_label_map`` once;
  * ``ops.reg_shift_labeled`` beside ``ops.reg_shift`` on the same stack, bilinear (fractional shifts) and nearest: the same bytes
    plus one label byte per pixel;
  * ``estimate_view_shifts`` and ``register_views`` whole, ``register_frames`` for comparison;
  * a float4 copy of 1 GiB (``Tensor.copy_``): the yardstick of the same run.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.  No ratio is fixed in advance: what comes out is recorded.
    python tools/register_views_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402


def lattice(L, pitch, H, W):
    """The L points of a hexagonal lattice of ``pitch`` pixels nearest to the middle of an H x W frame, as int32 (row, column)."""
    import numpy as np
    pts = []
    for r in range(-6, 7):
        for c in range(-6, 7):
            pts.append((r * pitch * 3 ** 0.5 / 2, (c + 0.5 * (r % 2)) * pitch))
    pts.sort(key=lambda p: (p[0] ** 2 + p[1] ** 2, p))
    return np.int32([[round(H / 2 + y), round(W / 2 + x)] for y, x in pts[:L]])


def measure(quick):
    import numpy as np
    import torch
    from cwfa_amd import ops
    from cwfa_amd.XLFMDataset import (estimate_view_shifts, fit_view_shifts, register_frames, register_views, taper_window, view_labels)
    N, H, W, L, side, pitch = (24, 512, 512, 7, 128, 150) if quick else (250, 2160, 2160, 29, 512, 380)
    P = H * W
    my = mx = 8
    taper, eps = 16, 1e-5
    centers = lattice(L, pitch, H, W)
    # directions in multiples of 8, at most 32 on the outer ring: a in {-1/8, 0, 1/8} plants integer shifts of at most 4 px
    gdir = 8.0 * np.round((centers - centers.mean(0)) / (pitch / 1.9))
    labels = view_labels((H, W), centers, (side, side))
    chunk = max(1, (256 << 20) // (L * side * side * 4))
    g = torch.Generator(device="cuda").manual_seed(5)
    base = torch.zeros(H, W, device="cuda")
    pts = torch.randint(0, P, (P // 400,), device="cuda", generator=g)
    base.view(-1)[pts] = 200.0 + 800.0 * torch.rand(pts.numel(), device="cuda", generator=g)
    k = torch.exp(-0.5 * (torch.arange(-4, 5, device="cuda", dtype=torch.float32) / 1.4) ** 2)
    base = torch.nn.functional.conv2d(base[None, None], (k[:, None] * k[None, :])[None, None], padding=4)[0, 0] + 120.0
    cpu = torch.Generator().manual_seed(1)
    d = torch.randint(-2, 3, (N, 2), generator=cpu).double()
    a = (torch.randint(-1, 2, (N,), generator=cpu).double()) / 8.0
    d[0], a[0] = 0.0, 0.0
    gd = torch.from_numpy(gdir)
    planted = torch.cat((d[:, None, :] + a[:, None, None] * gd[None], d[:, None, :]), dim=1).float().cuda()      # [N, L + 1, 2]
    x32 = torch.empty(N, H, W, device="cuda")
    for t in range(N):                                             # frame by frame: no second stack.  frame[p] = base[p - shift(label)]
        ops.reg_shift_labeled(base[None], -planted[t:t + 1], labels, mode="nearest", fill=120.0, out=x32[t:t + 1])
        x32[t] = torch.floor(x32[t] + 20.0 * torch.randn(H, W, device="cuda", generator=g))
    template = base.clone()
    stacks = {"fp32": x32, "fp16": x32.half()}
    wy, wx = taper_window(side, taper).cuda(), taper_window(side, taper).cuda()
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")
    fast, nbytes, checks = {"float4_copy": lambda: dst.copy_(src)}, {"float4_copy": 8 * n_copy}, {}
    fast["label_map"] = lambda: view_labels((H, W), centers, (side, side))
    kw = dict(max_shift=(my, mx), taper=taper, eps=eps)
    gdev = gd.cuda()
    rigid = planted[:, L].contiguous()
    for name, x in stacks.items():
        es = x.element_size()
        n = min(chunk, N)
        vw = ops.reg_window_views(x[:n], centers, (side, side), wy, wx)
        F = torch.fft.rfft2(vw).contiguous()
        T = torch.fft.rfft2(ops.reg_window_views(template[None], centers, (side, side), wy, wx)[0]).contiguous()
        Wt = torch.conj(ops.reg_whiten(T)).resolve_conj()
        R = ops.reg_whiten(F, Wt, eps)
        c = torch.fft.irfft2(R, s=(side, side)).reshape(n * L, side, side)
        shifts, peak = estimate_view_shifts(x, template, centers, (side, side), **kw)
        fit = fit_view_shifts(shifts, peak, gdev)
        out = torch.empty_like(x)
        frac = fit.table + 0.25
        fast[f"window_views_chunk_{name}"] = lambda x=x, vw=vw: ops.reg_window_views(x[:n], centers, (side, side), wy, wx, out=vw)
        fast[f"rfft2_chunk_{name}"] = lambda vw=vw: torch.fft.rfft2(vw)
        fast[f"whiten_chunk_{name}"] = lambda F=F, Wt=Wt, R=R: ops.reg_whiten(F, Wt, eps, out=R)
        fast[f"irfft2_chunk_{name}"] = lambda R=R: torch.fft.irfft2(R, s=(side, side))
        fast[f"peak_chunk_{name}"] = lambda c=c: ops.reg_peak(c, (my, mx))
        fast[f"fit_views_{name}"] = lambda shifts=shifts, peak=peak: ops.reg_fit_views(shifts, peak, gdev)
        fast[f"shift_labeled_bilinear_{name}"] = lambda x=x, frac=frac, out=out: ops.reg_shift_labeled(x, frac, labels, out=out)
        fast[f"shift_bilinear_{name}"] = lambda x=x, out=out: ops.reg_shift(x, rigid + 0.25, out=out)
        fast[f"shift_labeled_nearest_{name}"] = lambda x=x, fit=fit, out=out: ops.reg_shift_labeled(x, fit.table, labels, mode="nearest", out=out)
        fast[f"shift_nearest_{name}"] = lambda x=x, out=out: ops.reg_shift(x, rigid, mode="nearest", out=out)
        fast[f"estimate_view_shifts_{name}"] = lambda x=x: estimate_view_shifts(x, template, centers, (side, side), **kw)
        fast[f"register_views_{name}"] = lambda x=x, out=out: register_views(x, centers, (side, side), template=template, directions=gdev, labels=labels,
                                                                             out=out, **kw)
        fast[f"register_frames_{name}"] = lambda x=x, out=out: register_frames(x, template, out=out, max_shift=(my, mx), taper=taper, eps=eps)
        nbytes.update({f"window_views_chunk_{name}": n * L * side * side * (es + 4),
                       f"whiten_chunk_{name}": 16 * n * L * side * (side // 2 + 1) + 8 * L * side * (side // 2 + 1),
                       f"shift_labeled_bilinear_{name}": 2 * N * P * es + P, f"shift_labeled_nearest_{name}": 2 * N * P * es + P,
                       f"shift_bilinear_{name}": 2 * N * P * es, f"shift_nearest_{name}": 2 * N * P * es})
        want = torch.stack((d[:, 0], d[:, 1], a), dim=1)
        checks[f"planted_motion_recovered_{name}"] = round(float((fit.params.cpu() - want).abs().max()), 6)
        checks[f"inlier_fraction_{name}"] = round(float(fit.inlier.float().mean()), 4)
        checks[f"peak_min_{name}"] = round(float(peak.min()), 4)
        del vw, F, R, c
    ms = windows(fast, 3 if quick else 5, 1 if quick else 2, 1)
    res = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    copy_rate = res["float4_copy"]["GBps"]
    for k in nbytes:
        res[k]["fraction_of_measured_copy_rate"] = round(res[k]["GBps"] / copy_rate, 3)
        res[k]["ms_for_its_bytes_at_copy_rate"] = round(nbytes[k] / copy_rate / 1e6, 4)
    chunks = (N + chunk - 1) // chunk
    for name in stacks:
        fft = res[f"rfft2_chunk_{name}"]["ms"] + res[f"irfft2_chunk_{name}"]["ms"]
        ours = res[f"window_views_chunk_{name}"]["ms"] + res[f"whiten_chunk_{name}"]["ms"] + res[f"peak_chunk_{name}"]["ms"]
        res[f"transforms_share_of_a_chunk_{name}"] = round(fft / (fft + ours), 3)
        res[f"chunk_stages_sum_times_chunks_ms_{name}"] = round((fft + ours) * chunks, 3)
        for mode in ("bilinear", "nearest"):
            res[f"shift_labeled_over_shift_{mode}_{name}"] = round(res[f"shift_labeled_{mode}_{name}"]["ms"] / res[f"shift_{mode}_{name}"]["ms"], 3)
        res[f"register_views_over_register_frames_{name}"] = round(res[f"register_views_{name}"]["ms"] / res[f"register_frames_{name}"]["ms"], 2)
    res["checks"] = checks
    mixed = labels.view(H, W // 4, 4)
    res["config"] = {"stack": [N, H, W], "views": L, "view_shape": [side, side], "lattice_pitch": pitch, "chunk_frames": chunk, "max_shift": [my, mx],
                     "taper": taper, "eps": eps, "copy_elements": n_copy, "view_bytes_per_chunk": chunk * L * side * side * 4,
                     "pixels_in_a_view": round(float((labels < L).float().mean()), 4),
                     "groups_of_4_with_mixed_labels": round(float((mixed != mixed[..., :1]).any(-1).float().mean()), 6)}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "register_views_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "per-lenslet frame registration: cut-and-taper, transforms, whitened cross-power, peak, fit, labelled resampling, register_views",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "register_views": measure(quick)}
    out = os.path.join(ROOT, "profiles", "register_views_time_quick.json" if quick else "register_views_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["register_views"]))


if __name__ == "__main__":
    main()
