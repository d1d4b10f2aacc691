#!/usr/bin/env python3
"""Time the rigid registration of volumes on the MI355X and write profiles/register3d_time.json.

At 32 volumes of 96 x 512 x 512 (3.2 GB fp32; the workload's volume), one GPU process:

  * ``register_volumes`` (template given, one iteration, trilinear) and ``estimate_volume_shifts`` alone;
  * every stage of one volume: ``ops.reg_window3d``, the forward transform (``torch.fft.rfftn``), ``ops.reg_whiten``, the inverse
    transform (``torch.fft.irfftn``), ``ops.reg_peak3d``; and ``ops.reg_shift3d`` over the whole stack, trilinear (all three
    components fractional), in-plane only (an integer dz: one source plane) and nearest;
  * the same pipeline in torch operators on the same card: ``torch.fft``, elementwise complex operators, ``argmax`` over the rolled
    window (no sub-voxel step), 5-D ``grid_sample``;
  * a float4 copy of 1 GiB (``Tensor.copy_``): the yardstick.  Each new kernel's time is held against its bytes at that copy rate.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.  No ratio is fixed in advance: what comes out is recorded.
    python tools/register3d_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402


def torch_pipeline(x, template, wins, m, eps):
    """register_volumes in torch operators, volume by volume: integer peak only (no parabola), trilinear ``grid_sample``."""
    import torch
    N, D, H, W = x.shape
    mz, my, mx = m
    w3 = wins[0][:, None, None] * wins[1][None, :, None] * wins[2][None, None, :]
    T = torch.fft.rfftn(template * w3)
    Wt = torch.conj(T / (T.abs() + eps))
    Wt[0, 0, 0] = 0
    wh, ww = 2 * my + 1, 2 * mx + 1
    out = torch.empty_like(x)
    zs = torch.linspace(-1, 1, D, device=x.device)[:, None, None]
    ys = torch.linspace(-1, 1, H, device=x.device)[None, :, None]
    xs = torch.linspace(-1, 1, W, device=x.device)[None, None, :]
    shifts = torch.empty(N, 3, device=x.device)
    for n in range(N):
        F = torch.fft.rfftn(x[n] * w3)
        c = torch.fft.irfftn(F / (F.abs() + eps) * Wt, s=(D, H, W))
        win = torch.roll(c, (mz, my, mx), (0, 1, 2))[:2 * mz + 1, :wh, :ww]
        idx = win.reshape(-1).argmax()
        d = torch.stack((idx // (wh * ww) - mz, (idx // ww) % wh - my, idx % ww - mx)).to(torch.float32)
        shifts[n] = d
        gz = (zs + (2.0 / (D - 1)) * d[0]).expand(D, H, W)
        gy = (ys + (2.0 / (H - 1)) * d[1]).expand(D, H, W)
        gx = (xs + (2.0 / (W - 1)) * d[2]).expand(D, H, W)
        out[n] = torch.nn.functional.grid_sample(x[n][None, None], torch.stack((gx, gy, gz), -1)[None], mode="bilinear", padding_mode="zeros",
                                                 align_corners=True)[0, 0]
    return out, shifts


def measure(quick):
    import torch
    from cwfa_amd import ops
    from cwfa_amd.CWFA import estimate_volume_shifts, register_volumes
    from cwfa_amd.XLFMDataset import taper_window
    N, D, H, W = (6, 24, 64, 64) if quick else (32, 96, 512, 512)
    P, bins = D * H * W, D * H * (W // 2 + 1)
    m, eps = (2, 8, 8), 1e-5
    # the default taper; the quick form's 24 planes are a short axis, where it biases dz toward 0
    taper = (1, 8, 8) if quick else tuple(min(16, s // 8) for s in (D, H, W))
    g = torch.Generator(device="cuda").manual_seed(5)
    base = torch.zeros(D, H, W, device="cuda")
    pts = torch.randint(0, P, (P // 1000,), device="cuda", generator=g)
    base.view(-1)[pts] = 200.0 + 800.0 * torch.rand(pts.numel(), device="cuda", generator=g)
    k = torch.exp(-0.5 * (torch.arange(-4, 5, device="cuda", dtype=torch.float32) / 1.4) ** 2)
    for axis in range(3):                                          # a separable Gaussian: blobs of sigma 1.4 voxels
        shape = [1, 1, 1, 1, 1]
        shape[2 + axis] = 9
        pad = [0, 0, 0]
        pad[axis] = 4
        base = torch.nn.functional.conv3d(base[None, None], k.view(shape), padding=pad)[0, 0]
    base = base + 120.0
    planted = torch.stack([torch.randint(-v, v + 1, (N,), generator=torch.Generator().manual_seed(1 + a)) for a, v in enumerate((2, 6, 6))], 1)
    planted[0] = 0
    x = torch.empty(N, D, H, W, device="cuda")
    for t in range(N):                                             # volume by volume: no second stack
        x[t] = torch.floor(torch.roll(base, tuple(int(v) for v in planted[t]), (0, 1, 2)) + 20.0 * torch.randn(D, H, W, device="cuda", generator=g))
    template = base.clone()
    wins = tuple(taper_window(s, t).cuda() for s, t in zip((D, H, W), taper))
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")
    kw = dict(max_shift=m, taper=taper, eps=eps, chunk=1)
    xw = ops.reg_window3d(x[:1], *wins)
    F = torch.fft.rfftn(xw, dim=(-3, -2, -1)).contiguous()
    Wt = torch.conj(ops.reg_whiten(torch.fft.rfftn(ops.reg_window3d(template[None], *wins)[0]).contiguous())).resolve_conj()
    R = ops.reg_whiten(F, Wt, eps)
    c = torch.fft.irfftn(R, s=(D, H, W), dim=(-3, -2, -1))
    shifts, peak = estimate_volume_shifts(x, template, **kw)
    out = torch.empty_like(x)
    frac = shifts + 0.25
    inplane = frac.clone()
    inplane[:, 0] = shifts[:, 0]
    fast = {"float4_copy": lambda: dst.copy_(src),
            "window3d_volume": lambda: ops.reg_window3d(x[:1], *wins, out=xw),
            "rfftn_volume": lambda: torch.fft.rfftn(xw, dim=(-3, -2, -1)),
            "whiten_volume": lambda: ops.reg_whiten(F, Wt, eps, out=R),
            "irfftn_volume": lambda: torch.fft.irfftn(R, s=(D, H, W), dim=(-3, -2, -1)),
            "peak3d_volume": lambda: ops.reg_peak3d(c, m),
            "shift3d_trilinear": lambda: ops.reg_shift3d(x, frac, out=out),
            "shift3d_inplane": lambda: ops.reg_shift3d(x, inplane, out=out),
            "shift3d_nearest": lambda: ops.reg_shift3d(x, shifts, mode="nearest", out=out),
            "estimate_volume_shifts": lambda: estimate_volume_shifts(x, template, **kw),
            "register_volumes": lambda: register_volumes(x, template, out=out, **kw)}
    slow = {"torch_pipeline": lambda: torch_pipeline(x, template, wins, m, eps)}
    nbytes = {"float4_copy": 8 * n_copy, "window3d_volume": 8 * P, "whiten_volume": 16 * bins + 8 * bins,
              "shift3d_trilinear": 8 * N * P, "shift3d_inplane": 8 * N * P, "shift3d_nearest": 8 * N * P}
    checks = {"planted_shifts_recovered": bool(torch.equal(shifts.cpu().round().long(), planted)),
              "torch_pipeline_agrees": bool(torch.equal(torch_pipeline(x, template, wins, m, eps)[1].cpu().long(), planted)),
              "peak_min": round(float(peak.min()), 4)}
    ms = windows(fast, 3 if quick else 5, 1 if quick else 2, 1)
    ms.update(windows(slow, 2 if quick else 3, 1, 1))
    res = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    copy_rate = res["float4_copy"]["GBps"]
    for k in nbytes:
        res[k]["fraction_of_measured_copy_rate"] = round(res[k]["GBps"] / copy_rate, 3)
        res[k]["ms_for_its_bytes_at_copy_rate"] = round(nbytes[k] / copy_rate / 1e6, 4)
    fft = res["rfftn_volume"]["ms"] + res["irfftn_volume"]["ms"]
    ours = res["window3d_volume"]["ms"] + res["whiten_volume"]["ms"] + res["peak3d_volume"]["ms"]
    res["transforms_share_of_a_volume"] = round(fft / (fft + ours), 3)
    res["volume_stages_sum_times_volumes_ms"] = round((fft + ours) * N, 3)
    res["register_volumes_ms_per_volume"] = round(res["register_volumes"]["ms"] / N, 4)
    res["torch_pipeline_over_register_volumes"] = round(res["torch_pipeline"]["ms"] / res["register_volumes"]["ms"], 2)
    res["checks"] = checks
    res["config"] = {"stack": [N, D, H, W], "chunk": 1, "max_shift": list(m), "taper": list(taper), "eps": eps, "copy_elements": n_copy,
                     "spectrum_bytes_per_volume": 8 * bins}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "register3d_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "rigid registration of volumes: window, transforms, whitened cross-power, peak, resampling, register_volumes",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "register3d": measure(quick)}
    out = os.path.join(ROOT, "profiles", "register3d_time_quick.json" if quick else "register3d_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["register3d"]))


if __name__ == "__main__":
    main()
