#!/usr/bin/env python3
"""Time rigid frame registration on the MI355X and write profiles/register_time.json.

At 250 x 2160 x 2160 (the reference's raw stack: 4.7 GB fp32, 2.3 GB fp16), one GPU process, for fp32 and fp16:

  * ``register_frames`` (template given, one iteration, bilinear) and ``estimate_shifts`` alone;
  * every stage of one chunk of 16 frames: ``ops.reg_window``, the forward transform (``torch.fft.rfft2``), ``ops.reg_whiten``, the
    inverse transform (``torch.fft.irfft2``), ``ops.reg_peak``; and ``ops.reg_shift`` over the whole stack, bilinear and nearest;
  * the same pipeline in torch operators on the same card: ``torch.fft``, elementwise complex operators, ``argmax`` over the rolled
    window (no sub-pixel step), ``grid_sample``;
  * a float4 copy of 1 GiB (``Tensor.copy_``): the yardstick.  Each new kernel's time is held against its bytes at that copy rate.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.  No ratio is fixed in advance: what comes out is recorded.
    python tools/register_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402

CHUNK = 16


def torch_pipeline(x, template, wy, wx, my, mx, eps):
    """register_frames in torch operators, chunk by chunk: integer peak only (no parabola), bilinear ``grid_sample``."""
    import torch
    N, H, W = x.shape
    w2 = wy[:, None] * wx[None, :]
    T = torch.fft.rfft2(template * w2)
    Wt = torch.conj(T / (T.abs() + eps))
    Wt[0, 0] = 0
    ww = 2 * mx + 1
    out = torch.empty_like(x)
    ys = torch.linspace(-1, 1, H, device=x.device)[None, :, None]
    xs = torch.linspace(-1, 1, W, device=x.device)[None, None, :]
    shifts = torch.empty(N, 2, device=x.device)
    for s in range(0, N, CHUNK):
        e = min(s + CHUNK, N)
        F = torch.fft.rfft2(x[s:e].float() * w2)
        c = torch.fft.irfft2(F / (F.abs() + eps) * Wt, s=(H, W))
        win = torch.roll(c, (my, mx), (1, 2))[:, :2 * my + 1, :ww]
        idx = win.reshape(e - s, -1).argmax(1)
        d = torch.stack((idx // ww - my, idx % ww - mx), 1).to(torch.float32)
        shifts[s:e] = d
        gy = (ys + (2.0 / (H - 1)) * d[:, 0, None, None]).expand(e - s, H, W)
        gx = (xs + (2.0 / (W - 1)) * d[:, 1, None, None]).expand(e - s, H, W)
        out[s:e] = torch.nn.functional.grid_sample(x[s:e, None].float(), torch.stack((gx, gy), -1), mode="bilinear", padding_mode="zeros",
                                                   align_corners=True)[:, 0]                 # fp16: sampled in fp32, a half grid cannot address 2160 px
    return out, shifts


def measure(quick):
    import torch
    from cwfa_amd import ops
    from cwfa_amd.XLFMDataset import estimate_shifts, register_frames, taper_window
    N, H, W = (48, 256, 256) if quick else (250, 2160, 2160)
    P, bins = H * W, H * (W // 2 + 1)
    my = mx = 16
    taper, eps = 16, 1e-5
    g = torch.Generator(device="cuda").manual_seed(5)
    base = torch.zeros(H, W, device="cuda")
    pts = torch.randint(0, P, (P // 400,), device="cuda", generator=g)
    base.view(-1)[pts] = 200.0 + 800.0 * torch.rand(pts.numel(), device="cuda", generator=g)
    k = torch.exp(-0.5 * (torch.arange(-4, 5, device="cuda", dtype=torch.float32) / 1.4) ** 2)
    base = torch.nn.functional.conv2d(base[None, None], (k[:, None] * k[None, :])[None, None], padding=4)[0, 0] + 120.0
    planted = torch.randint(-6, 7, (N, 2), generator=torch.Generator().manual_seed(1))
    planted[0] = 0
    x32 = torch.empty(N, H, W, device="cuda")
    for t in range(N):                                             # frame by frame: no second stack
        x32[t] = torch.floor(torch.roll(base, tuple(int(v) for v in planted[t]), (0, 1)) + 20.0 * torch.randn(H, W, device="cuda", generator=g))
    template = base.clone()
    stacks = {"fp32": x32, "fp16": x32.half()}
    wy, wx = taper_window(H, taper).cuda(), taper_window(W, taper).cuda()
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")
    fast, slow, nbytes, checks = {"float4_copy": lambda: dst.copy_(src)}, {}, {"float4_copy": 8 * n_copy}, {}
    kw = dict(max_shift=(my, mx), taper=taper, eps=eps, chunk=CHUNK)
    for name, x in stacks.items():
        es = x.element_size()
        n = min(CHUNK, N)
        xw = ops.reg_window(x[:n], wy, wx)
        F = torch.fft.rfft2(xw).contiguous()
        Wt = torch.conj(ops.reg_whiten(torch.fft.rfft2(ops.reg_window(template[None], wy, wx)[0]).contiguous())).resolve_conj()
        R = ops.reg_whiten(F, Wt, eps)
        c = torch.fft.irfft2(R, s=(H, W))
        shifts, peak = estimate_shifts(x, template, **kw)
        out = torch.empty_like(x)
        fast[f"window_chunk_{name}"] = lambda x=x, xw=xw: ops.reg_window(x[:n], wy, wx, out=xw)
        fast[f"rfft2_chunk_{name}"] = lambda xw=xw: torch.fft.rfft2(xw)
        fast[f"whiten_chunk_{name}"] = lambda F=F, Wt=Wt, R=R: ops.reg_whiten(F, Wt, eps, out=R)
        fast[f"irfft2_chunk_{name}"] = lambda R=R: torch.fft.irfft2(R, s=(H, W))
        fast[f"peak_chunk_{name}"] = lambda c=c: ops.reg_peak(c, (my, mx))
        fast[f"shift_bilinear_{name}"] = lambda x=x, shifts=shifts, out=out: ops.reg_shift(x, shifts + 0.25, out=out)
        fast[f"shift_nearest_{name}"] = lambda x=x, shifts=shifts, out=out: ops.reg_shift(x, shifts, mode="nearest", out=out)
        fast[f"estimate_shifts_{name}"] = lambda x=x: estimate_shifts(x, template, **kw)
        fast[f"register_frames_{name}"] = lambda x=x, out=out: register_frames(x, template, out=out, **kw)
        slow[f"torch_pipeline_{name}"] = lambda x=x: torch_pipeline(x, template, wy, wx, my, mx, eps)
        nbytes.update({f"window_chunk_{name}": n * P * (es + 4), f"whiten_chunk_{name}": 16 * n * bins + 8 * bins,
                       f"shift_bilinear_{name}": 2 * N * P * es, f"shift_nearest_{name}": 2 * N * P * es})
        checks[f"planted_shifts_recovered_{name}"] = bool(torch.equal(shifts.cpu().round().long(), planted))
        checks[f"torch_pipeline_agrees_{name}"] = bool(torch.equal(torch_pipeline(x, template, wy, wx, my, mx, eps)[1].cpu().long(), planted))
        checks[f"peak_min_{name}"] = round(float(peak.min()), 4)
        del xw, F, R, c
    ms = windows(fast, 3 if quick else 5, 1 if quick else 2, 1)
    ms.update(windows(slow, 2 if quick else 3, 1, 1))
    res = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    copy_rate = res["float4_copy"]["GBps"]
    for k in nbytes:
        res[k]["fraction_of_measured_copy_rate"] = round(res[k]["GBps"] / copy_rate, 3)
        res[k]["ms_for_its_bytes_at_copy_rate"] = round(nbytes[k] / copy_rate / 1e6, 4)
    chunks = (N + CHUNK - 1) // CHUNK
    for name in stacks:
        fft = res[f"rfft2_chunk_{name}"]["ms"] + res[f"irfft2_chunk_{name}"]["ms"]
        ours = res[f"window_chunk_{name}"]["ms"] + res[f"whiten_chunk_{name}"]["ms"] + res[f"peak_chunk_{name}"]["ms"]
        res[f"transforms_share_of_a_chunk_{name}"] = round(fft / (fft + ours), 3)
        res[f"chunk_stages_sum_times_chunks_ms_{name}"] = round((fft + ours) * chunks, 3)
        res[f"torch_pipeline_over_register_frames_{name}"] = round(res[f"torch_pipeline_{name}"]["ms"] / res[f"register_frames_{name}"]["ms"], 2)
    res["checks"] = checks
    res["config"] = {"stack": [N, H, W], "chunk": CHUNK, "max_shift": [my, mx], "taper": taper, "eps": eps, "copy_elements": n_copy,
                     "spectrum_bytes_per_frame": 8 * bins}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "register_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "rigid frame registration: window, transforms, whitened cross-power, peak, resampling, register_frames",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "register": measure(quick)}
    out = os.path.join(ROOT, "profiles", "register_time_quick.json" if quick else "register_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["register"]))


if __name__ == "__main__":
    main()
