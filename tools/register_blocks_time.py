#!/usr/bin/env python3
"""Time the piecewise-rigid registration of volumes on the MI355X and write profiles/register_blocks_time.json.

At 32 volumes of 96 x 512 x 512 (3.2 GB fp32; the shape of section 30.5), grid (3, 4, 4), blocks of 32 x 128 x 128, one GPU process:

  * ``ops.reg_warp3d`` over the whole stack -- a fractional field, a constant one and nearest -- beside ``ops.reg_shift3d`` (all three
    components fractional) and beside a float4 copy of 1 GiB (``Tensor.copy_``), the yardstick of the same session;
  * every stage of one volume: the three new ones (``ops.reg_window_blocks3d``, ``ops.reg_field_fill``, ``ops.reg_warp3d``) and the
    reused ones on the batch of 48 blocks (``torch.fft.rfftn``, ``ops.reg_whiten``, ``torch.fft.irfftn``, ``ops.reg_peak3d``);
  * ``register_volumes_piecewise`` and ``estimate_block_shifts`` (with the base given, and with the default whole-volume base)
    beside ``register_volumes``.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.  No ratio is fixed in advance: what comes out is recorded.
    python tools/register_blocks_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402


def measure(quick):
    import torch
    from cwfa_amd import ops
    from cwfa_amd.CWFA import block_grid, estimate_block_shifts, register_volumes, register_volumes_piecewise
    N, D, H, W = (6, 24, 64, 64) if quick else (32, 96, 512, 512)
    block, grid = ((8, 16, 16), (3, 4, 4)) if quick else ((32, 128, 128), (3, 4, 4))
    P = D * H * W
    m, eps = (2, 4, 4) if quick else (2, 8, 8), 1e-5
    G = block_grid((D, H, W), block, grid, device="cuda")
    B, Pb = G.B, block[0] * block[1] * block[2]
    bins = block[0] * block[1] * (block[2] // 2 + 1)
    taper = tuple(min(16, s // 8) for s in block)
    g = torch.Generator(device="cuda").manual_seed(5)
    base_vol = torch.zeros(D, H, W, device="cuda")
    pts = torch.randint(0, P, (P // 1000,), device="cuda", generator=g)
    base_vol.view(-1)[pts] = 200.0 + 800.0 * torch.rand(pts.numel(), device="cuda", generator=g)
    k = torch.exp(-0.5 * (torch.arange(-4, 5, device="cuda", dtype=torch.float32) / 1.4) ** 2)
    for axis in range(3):                                          # a separable Gaussian: blobs of sigma 1.4 voxels
        shape = [1, 1, 1, 1, 1]
        shape[2 + axis] = 9
        pad = [0, 0, 0]
        pad[axis] = 4
        base_vol = torch.nn.functional.conv3d(base_vol[None, None], k.view(shape), padding=pad)[0, 0]
    base_vol = base_vol + 120.0
    planted = torch.stack([torch.randint(-v, v + 1, (N,), generator=torch.Generator().manual_seed(1 + a)) for a, v in enumerate((1, 3, 3))], 1)
    planted[0] = 0
    x = torch.empty(N, D, H, W, device="cuda")
    for t in range(N):                                             # volume by volume: no second stack
        x[t] = torch.floor(torch.roll(base_vol, tuple(int(v) for v in planted[t]), (0, 1, 2)) + 20.0 * torch.randn(D, H, W, device="cuda", generator=g))
    template = base_vol.clone()
    wins = G.windows(taper, "cuda")
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")
    kw = dict(max_shift=m, taper=taper, eps=eps, chunk=1)
    xb = ops.reg_window_blocks3d(x[:1], G.origins, block, *wins)
    F = torch.fft.rfftn(xb, dim=(-3, -2, -1)).contiguous()
    Wt = torch.conj(ops.reg_whiten(torch.fft.rfftn(ops.reg_window_blocks3d(template[None], G.origins, block, *wins)[0], dim=(-3, -2, -1)).contiguous())).resolve_conj()
    R = ops.reg_whiten(F, Wt, eps)
    c = torch.fft.irfftn(R, s=block, dim=(-3, -2, -1)).reshape(B, *block)
    zero = torch.zeros(N, 3, device="cuda")
    field, peak, inlier = estimate_block_shifts(x, template, G, base=zero, **kw)
    raw, pk1 = field.reshape(N, B, 3), peak.reshape(N, B)
    out = torch.empty_like(x)
    tabs = G.tables("cuda")
    frac = (field.reshape(N, B, 3) + 0.5 * torch.rand(N, B, 3, device="cuda", generator=g)).contiguous()
    const = frac[:, :1].expand(N, B, 3).contiguous()
    rigid = frac[:, 0].contiguous()
    ff, fi = ops.reg_field_fill(raw, pk1, zero, grid, 0.0, None)
    fast = {"float4_copy": lambda: dst.copy_(src),
            "window_blocks_volume": lambda: ops.reg_window_blocks3d(x[:1], G.origins, block, *wins, out=xb),
            "rfftn_blocks_volume": lambda: torch.fft.rfftn(xb, dim=(-3, -2, -1)),
            "whiten_blocks_volume": lambda: ops.reg_whiten(F, Wt, eps, out=R),
            "irfftn_blocks_volume": lambda: torch.fft.irfftn(R, s=block, dim=(-3, -2, -1)),
            "peak3d_blocks_volume": lambda: ops.reg_peak3d(c, m),
            "field_fill_stack": lambda: ops.reg_field_fill(raw, pk1, zero, grid, 0.1, (1.0, 2.0, 2.0), out=(ff, fi)),
            "warp3d_volume": lambda: ops.reg_warp3d(x[:1], frac[:1], grid, tabs, out=out[:1]),
            "warp3d_fractional": lambda: ops.reg_warp3d(x, frac, grid, tabs, out=out),
            "warp3d_constant": lambda: ops.reg_warp3d(x, const, grid, tabs, out=out),
            "warp3d_nearest": lambda: ops.reg_warp3d(x, frac, grid, tabs, mode="nearest", out=out),
            "shift3d_trilinear": lambda: ops.reg_shift3d(x, rigid, out=out),
            "estimate_block_shifts_base_given": lambda: estimate_block_shifts(x, template, G, base=zero, **kw),
            "estimate_block_shifts": lambda: estimate_block_shifts(x, template, G, **kw),
            "register_volumes_piecewise": lambda: register_volumes_piecewise(x, template, grid=G, out=out, **kw),
            "register_volumes": lambda: register_volumes(x, template, out=out, **kw)}
    nbytes = {"float4_copy": 8 * n_copy, "window_blocks_volume": 8 * B * Pb, "whiten_blocks_volume": 24 * B * bins, "warp3d_volume": 8 * P,
              "warp3d_fractional": 8 * N * P, "warp3d_constant": 8 * N * P, "warp3d_nearest": 8 * N * P, "shift3d_trilinear": 8 * N * P}
    want = planted[:, None, :].expand(N, B, 3)
    checks = {"planted_shifts_recovered_in_every_block": bool(torch.equal(field.reshape(N, B, 3).cpu().round().long(), want)),
              "all_inliers": bool(inlier.all()), "peak_min": round(float(peak.min()), 4),
              "constant_field_is_shift3d": bool(torch.equal(ops.reg_warp3d(x[:2], const[:2], grid, tabs).view(torch.int32),
                                                            ops.reg_shift3d(x[:2], rigid[:2]).view(torch.int32)))}
    ms = windows(fast, 3 if quick else 5, 1 if quick else 2, 1)
    res = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    copy_rate = res["float4_copy"]["GBps"]
    for k in nbytes:
        res[k]["fraction_of_measured_copy_rate"] = round(res[k]["GBps"] / copy_rate, 3)
        res[k]["ms_for_its_bytes_at_copy_rate"] = round(nbytes[k] / copy_rate / 1e6, 4)
    fft = res["rfftn_blocks_volume"]["ms"] + res["irfftn_blocks_volume"]["ms"]
    ours = res["window_blocks_volume"]["ms"] + res["whiten_blocks_volume"]["ms"] + res["peak3d_blocks_volume"]["ms"]
    res["transforms_share_of_a_volume_estimate"] = round(fft / (fft + ours), 3)
    res["volume_stages_sum_ms"] = round(fft + ours + res["warp3d_volume"]["ms"] + res["field_fill_stack"]["ms"] / N, 4)
    res["warp3d_over_shift3d"] = round(res["warp3d_fractional"]["ms"] / res["shift3d_trilinear"]["ms"], 3)
    res["register_volumes_piecewise_ms_per_volume"] = round(res["register_volumes_piecewise"]["ms"] / N, 4)
    res["register_volumes_ms_per_volume"] = round(res["register_volumes"]["ms"] / N, 4)
    res["piecewise_over_rigid"] = round(res["register_volumes_piecewise"]["ms"] / res["register_volumes"]["ms"], 3)
    res["checks"] = checks
    res["config"] = {"stack": [N, D, H, W], "grid": list(grid), "block": list(block), "chunk": 1, "max_shift": list(m), "taper": list(taper), "eps": eps,
                     "copy_elements": n_copy, "block_voxels_over_volume_voxels": round(B * Pb / P, 3)}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "register_blocks_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "piecewise-rigid registration of volumes: block cut, transforms, whitened cross-power, peak, field clean-up, warp",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "register_blocks": measure(quick)}
    out = os.path.join(ROOT, "profiles", "register_blocks_time_quick.json" if quick else "register_blocks_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["register_blocks"]))


if __name__ == "__main__":
    main()
