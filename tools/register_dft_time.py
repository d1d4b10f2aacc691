#!/usr/bin/env python3
"""Time the up-sampled-DFT refinement of rigid frame registration on the MI355X and write
profiles/register_dft_time.json.

At 250 x 2160 x 2160 fp32, chunks of 16, max_shift 16, taper 16, one GPU process:

  * ``estimate_shifts`` with ``subpixel=True`` (the parabola: the path of section 26.3, timed again here) against
    ``subpixel="dft"`` at ``upsample`` 16 and 4;
  * on one chunk of 16 whitened spectra, at either factor: ``ops.reg_upsample`` whole, and its twiddle, row and column kernels alone
    (the measurement-only option "reg_upsample_stages"), ``ops.reg_fine_peak``, and ``ops.reg_peak`` beside them;
  * a float4 copy of 1 GiB (``Tensor.copy_``): the yardstick.  The row kernel reads the chunk's spectra once; its time is held
    against those bytes at the copy rate of this run.
  * whether ``torch.fft.irfft2`` leaves the chunk's spectra as they were, at this size.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.  No number is fixed in advance: what comes out is recorded.
    python tools/register_dft_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402

CHUNK = 16
FACTORS = (16, 4)


def measure(quick):
    import torch
    from cwfa_amd import _lib, ops
    from cwfa_amd.XLFMDataset import estimate_shifts, taper_window
    L = _lib.lib()
    N, H, W = (48, 256, 256) if quick else (250, 2160, 2160)
    P, K = H * W, W // 2 + 1
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
    x = torch.empty(N, H, W, device="cuda")
    for t in range(N):                                             # frame by frame: no second stack
        x[t] = torch.floor(torch.roll(base, tuple(int(v) for v in planted[t]), (0, 1)) + 20.0 * torch.randn(H, W, device="cuda", generator=g))
    template = base.clone()
    wy, wx = taper_window(H, taper).cuda(), taper_window(W, taper).cuda()
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")
    kw = dict(max_shift=(my, mx), taper=taper, eps=eps, chunk=CHUNK)
    n = min(CHUNK, N)
    F = torch.fft.rfft2(ops.reg_window(x[:n], wy, wx)).contiguous()
    Wt = torch.conj(ops.reg_whiten(torch.fft.rfft2(ops.reg_window(template[None], wy, wx)[0]).contiguous())).resolve_conj()
    R = ops.reg_whiten(F, Wt, eps)
    before = R.clone()
    c = torch.fft.irfft2(R, s=(H, W))
    checks = {"irfft2_leaves_its_input_alone": bool(torch.equal(torch.view_as_real(R), torch.view_as_real(before)))}
    del before, F
    shifts, ipeak, peak = ops.reg_peak(c, (my, mx), False)
    fast = {"float4_copy": lambda: dst.copy_(src), "peak_chunk": lambda: ops.reg_peak(c, (my, mx)),
            "estimate_shifts_parabola": lambda: estimate_shifts(x, template, subpixel=True, **kw)}
    nbytes = {"float4_copy": 8 * n_copy}

    def staged(mask, u, C, ws):
        def run():
            L.cwfa_set_option(b"reg_upsample_stages", mask)
            ops.reg_upsample(R, ipeak, (H, W), u, out=C, workspace=ws)
            L.cwfa_set_option(b"reg_upsample_stages", 7)
        return run

    for u in FACTORS:
        U = 2 * u + 1
        C = ops.reg_upsample(R, ipeak, (H, W), u)
        ws = torch.empty(16 * n * U * (K + 2 * H) // 8, dtype=torch.float64, device="cuda")
        sh, pk = shifts.clone(), peak.clone()
        fast[f"upsample_chunk_u{u}"] = staged(7, u, C, ws)
        fast[f"twiddles_chunk_u{u}"] = staged(1, u, C, ws)
        fast[f"rows_chunk_u{u}"] = staged(2, u, C, ws)
        fast[f"columns_chunk_u{u}"] = staged(4, u, C, ws)
        fast[f"fine_peak_chunk_u{u}"] = lambda C=C, sh=sh, pk=pk, u=u: ops.reg_fine_peak(C, ipeak, u, out=(sh, pk))
        fast[f"estimate_shifts_dft_u{u}"] = lambda u=u: estimate_shifts(x, template, subpixel="dft", upsample=u, **kw)
        nbytes[f"rows_chunk_u{u}"] = 8 * n * H * K
        s_dft, _ = estimate_shifts(x, template, subpixel="dft", upsample=u, **kw)
        checks[f"planted_shifts_recovered_u{u}"] = bool(torch.equal(s_dft.cpu().round().long(), planted))
        checks[f"largest_distance_from_planted_px_u{u}"] = round(float((s_dft.cpu() - planted).abs().max()), 6)
    s_par, _ = estimate_shifts(x, template, subpixel=True, **kw)
    checks["largest_distance_from_planted_px_parabola"] = round(float((s_par.cpu() - planted).abs().max()), 6)
    ms = windows(fast, 3 if quick else 5, 1 if quick else 2, 1)
    res = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    copy_rate = res["float4_copy"]["GBps"]
    chunks = (N + CHUNK - 1) // CHUNK
    for u in FACTORS:
        r = res[f"rows_chunk_u{u}"]
        r["ms_for_its_bytes_at_copy_rate"] = round(r["bytes_algorithmic"] / copy_rate / 1e6, 4)
        r["times_its_byte_floor"] = round(r["ms"] / r["ms_for_its_bytes_at_copy_rate"], 2)
        U = 2 * u + 1
        r["float64_operations"] = 8 * n * H * K * U                  # four products, a difference, a sum, two accumulations per bin and column
        r["float64_Gop_per_s"] = round(r["float64_operations"] / r["ms"] / 1e6, 1)
        res[f"dft_over_parabola_u{u}"] = round(res[f"estimate_shifts_dft_u{u}"]["ms"] / res["estimate_shifts_parabola"]["ms"], 3)
        res[f"upsample_and_fine_peak_times_chunks_ms_u{u}"] = round((res[f"upsample_chunk_u{u}"]["ms"] + res[f"fine_peak_chunk_u{u}"]["ms"]) * chunks, 3)
    res["checks"] = checks
    res["config"] = {"stack": [N, H, W], "chunk": CHUNK, "max_shift": [my, mx], "taper": taper, "eps": eps, "copy_elements": n_copy,
                     "spectrum_bytes_per_frame": 8 * H * K, "factors": list(FACTORS)}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "register_dft_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "up-sampled-DFT refinement of rigid frame registration: estimate_shifts by parabola and by dft, the kernels of a chunk",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "register_dft": measure(quick)}
    out = os.path.join(ROOT, "profiles", "register_dft_time_quick.json" if quick else "register_dft_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["register_dft"]))


if __name__ == "__main__":
    main()
