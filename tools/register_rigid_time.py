#!/usr/bin/env python3
"""Time the rigid registration of volumes with a rotation about the optical axis on the MI355X and write
profiles/register_rigid_time.json.

At 32 volumes of 96 x 512 x 512 (3.2 GB fp32; the shape of sections 30.5 and 32.5), grid (3, 4, 4), blocks of 32 x 128 x 128, one GPU
process:

  * ``ops.reg_rigid3d`` over the whole stack at 0, 2 and 10 degrees (fractional shifts) and nearest, beside ``ops.reg_shift3d`` (all
    three components fractional), ``ops.reg_warp3d`` (a fractional field) and a float4 copy of 1 GiB (``Tensor.copy_``), the yardstick
    of the same session;
  * ``ops.reg_fit_rigid`` on the stack's table, with and without a prior;
  * ``estimate_rigid_motion`` with 0, 1 and 2 refinement passes (their differences are the cost of a pass);
  * ``register_volumes_rigid`` beside ``register_volumes`` and ``register_volumes_piecewise``.

The scene is the blob volume of tools/register_blocks_time.py turned by a planted angle of up to 2 degrees and moved by a planted
sub-voxel shift per volume; whether the planted motion comes back is recorded.  Every form is warmed up; HIP events around windows of
calls; the forms alternate inside one process; median (min, max) over the windows.  No ratio is fixed in advance: what comes out is
recorded.
    python tools/register_rigid_time.py [--quick]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402


def measure(quick):
    import torch
    from cwfa_amd import ops
    from cwfa_amd.CWFA import (block_grid, estimate_rigid_motion, register_volumes, register_volumes_piecewise, register_volumes_rigid, rigid_angles)
    N, D, H, W = (6, 24, 64, 64) if quick else (32, 96, 512, 512)
    block, grid = ((8, 16, 16), (3, 4, 4)) if quick else ((32, 128, 128), (3, 4, 4))
    P = D * H * W
    m, eps = (2, 4, 4) if quick else (2, 8, 8), 1e-5
    G = block_grid((D, H, W), block, grid, device="cuda")
    B = G.B
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
    hg = torch.Generator().manual_seed(1)
    max_deg = 2.0 if not quick else 1.0
    theta = (torch.rand(N, generator=hg, dtype=torch.float64) * 2 - 1) * math.radians(max_deg)
    d = (torch.rand(N, 2, generator=hg, dtype=torch.float64) * 2 - 1) * 2.0
    theta[0], d[0] = 0.0, 0.0
    c, s = torch.cos(theta), torch.sin(theta)
    planted = torch.stack((torch.zeros(N, dtype=torch.float64), d[:, 0], d[:, 1], c, s), 1)
    # volume n is the template under the inverse of planted[n]: rotation -theta, shift -R^T d
    inverse = torch.stack((torch.zeros(N, dtype=torch.float64), -(c * d[:, 0] + s * d[:, 1]), -(-s * d[:, 0] + c * d[:, 1]), c, -s), 1).cuda()
    x = torch.empty(N, D, H, W, device="cuda")
    for t in range(N):                                             # volume by volume: no second stack
        ops.reg_rigid3d(base_vol[None], inverse[t:t + 1], fill=120.0, out=x[t:t + 1])
        x[t] = torch.floor(x[t] + 20.0 * torch.randn(D, H, W, device="cuda", generator=g))
    template = base_vol.clone()
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=g), torch.empty(n_copy, device="cuda")
    kw = dict(max_shift=m, taper=taper, eps=eps, chunk=1)
    out = torch.empty_like(x)
    tabs = G.tables("cuda")
    frac = (torch.rand(N, B, 3, device="cuda", generator=g) * 3.0 - 1.5).contiguous()
    vec = frac[:, 0].contiguous()

    def turned(deg):
        th = torch.full((N,), math.radians(deg), dtype=torch.float64)
        th[1::2] *= -1
        return torch.cat((vec.cpu().double(), torch.cos(th)[:, None], torch.sin(th)[:, None]), 1).cuda()

    p0, p2, p10 = turned(0.0), turned(2.0), turned(10.0)
    params, peak, inlier, shifts = estimate_rigid_motion(x, template, G, n_refine=2, **kw)
    raw, pk1 = shifts.reshape(N, B, 3).contiguous(), peak.reshape(N, B).contiguous()
    from cwfa_amd.CWFA import _rigid_arms, _rigid_center
    arms = _rigid_arms(G, _rigid_center(None, (D, H, W), "tool"), "cuda")
    fast = {"float4_copy": lambda: dst.copy_(src),
            "rigid3d_0deg": lambda: ops.reg_rigid3d(x, p0, out=out),
            "rigid3d_2deg": lambda: ops.reg_rigid3d(x, p2, out=out),
            "rigid3d_10deg": lambda: ops.reg_rigid3d(x, p10, out=out),
            "rigid3d_2deg_nearest": lambda: ops.reg_rigid3d(x, p2, mode="nearest", out=out),
            "rigid3d_2deg_volume": lambda: ops.reg_rigid3d(x[:1], p2[:1], out=out[:1]),
            "shift3d_trilinear": lambda: ops.reg_shift3d(x, vec, out=out),
            "warp3d_fractional": lambda: ops.reg_warp3d(x, frac, grid, tabs, out=out),
            "fit_rigid_stack": lambda: ops.reg_fit_rigid(raw, pk1, arms, 0.0, 1.0),
            "fit_rigid_stack_prior": lambda: ops.reg_fit_rigid(raw, pk1, arms, 0.0, 1.0, prior=params)}
    slow = {"estimate_rigid_motion_0_refine": lambda: estimate_rigid_motion(x, template, G, n_refine=0, **kw),
            "estimate_rigid_motion_1_refine": lambda: estimate_rigid_motion(x, template, G, n_refine=1, **kw),
            "estimate_rigid_motion_2_refine": lambda: estimate_rigid_motion(x, template, G, n_refine=2, **kw),
            "register_volumes_rigid": lambda: register_volumes_rigid(x, template, grid=G, n_refine=2, out=out, **kw),
            "register_volumes_piecewise": lambda: register_volumes_piecewise(x, template, grid=G, out=out, **kw),
            "register_volumes": lambda: register_volumes(x, template, out=out, **kw)}
    nbytes = {"float4_copy": 8 * n_copy, "rigid3d_0deg": 8 * N * P, "rigid3d_2deg": 8 * N * P, "rigid3d_10deg": 8 * N * P, "rigid3d_2deg_nearest": 8 * N * P,
              "rigid3d_2deg_volume": 8 * P, "shift3d_trilinear": 8 * N * P, "warp3d_fractional": 8 * N * P}
    got = params.cpu()
    angle_err = (rigid_angles(got) - rigid_angles(planted)).abs()
    checks = {"planted_max_deg": max_deg, "largest_angle_error_deg": round(float(angle_err.max()), 5),
              "largest_shift_error_voxels": round(float((got[:, :3] - planted[:, :3]).abs().max()), 5),
              "inliers": int(inlier.sum()), "blocks": int(inlier.numel()), "peak_min": round(float(peak.min()), 4),
              "no_rotation_is_shift3d": bool(torch.equal(ops.reg_rigid3d(x[:2], p0[:2]).view(torch.int32), ops.reg_shift3d(x[:2], vec[:2]).view(torch.int32)))}
    ms = windows(fast, 3 if quick else 5, 1 if quick else 2, 1)
    ms.update(windows(slow, 3, 1, 1))
    res = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
    copy_rate = res["float4_copy"]["GBps"]
    for k in nbytes:
        res[k]["fraction_of_measured_copy_rate"] = round(res[k]["GBps"] / copy_rate, 3)
        res[k]["ms_for_its_bytes_at_copy_rate"] = round(nbytes[k] / copy_rate / 1e6, 4)
    for k in ("rigid3d_0deg", "rigid3d_2deg", "rigid3d_10deg"):
        res[k + "_over_shift3d"] = round(res[k]["ms"] / res["shift3d_trilinear"]["ms"], 3)
        res[k + "_over_warp3d"] = round(res[k]["ms"] / res["warp3d_fractional"]["ms"], 3)
    res["refinement_pass_ms_per_volume"] = round((res["estimate_rigid_motion_2_refine"]["ms"] - res["estimate_rigid_motion_0_refine"]["ms"]) / 2 / N, 4)
    res["first_pass_ms_per_volume"] = round(res["estimate_rigid_motion_0_refine"]["ms"] / N, 4)
    for k in ("register_volumes_rigid", "register_volumes_piecewise", "register_volumes"):
        res[k + "_ms_per_volume"] = round(res[k]["ms"] / N, 4)
    res["rigid_over_translation_only"] = round(res["register_volumes_rigid"]["ms"] / res["register_volumes"]["ms"], 3)
    res["rigid_over_piecewise"] = round(res["register_volumes_rigid"]["ms"] / res["register_volumes_piecewise"]["ms"], 3)
    res["checks"] = checks
    res["config"] = {"stack": [N, D, H, W], "grid": list(grid), "block": list(block), "chunk": 1, "n_refine": 2, "max_shift": list(m), "taper": list(taper),
                     "eps": eps, "copy_elements": n_copy}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "register_rigid_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "rigid registration of volumes with rotation about z: block table, rigid fit, refinement passes, one rigid resampling",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "register_rigid": measure(quick)}
    out = os.path.join(ROOT, "profiles", "register_rigid_time_quick.json" if quick else "register_rigid_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["register_rigid"]))


if __name__ == "__main__":
    main()
