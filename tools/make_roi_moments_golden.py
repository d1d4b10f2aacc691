"""Write the ROI-moments fixture tests/golden/g26_roi_moments.npz: TWO stacked CAT steps built by the REFERENCE's own
conditional_wavelet_flow (imported by oracle.make_golden's recipe; n_ch = 8, cond_ch = 4 as tests/test_host_logic.build_step;
D = 8, H = 12, W = 16, B = 2: step index 1 is the coarser step with C = 2 detail channels, step index 0 the finer one with C = 4),
cast to float64, with seeded conditions and coarsest low band.  State dicts, inputs and recorded results only.  Run from the
repository root:
    python tools/make_roi_moments_golden.py

The reference has no ROI-moment function.  It fixes the MAP from the latents of both steps to the volume, and the moments of an ROI
mean follow from that map by the reference's autograd: for independent latents of unit variance
    var_unit[b, r] = sum over both steps' latents of (d mean_r / d z)^2
    cov_unit[b, p] = (d mean_r1 / d z) . (d mean_r2 / d z)
(the volume is affine in z, so the gradients do not depend on where they are taken: z = 0 here).

Arrays: s0/*, s1/* per step index (sd/* the state dict, fp32 as built; meta/axis_i the PermuteDim axes; c0, c1 the conditions, fp32 as
drawn), low (fp32), boxes, pairs (tests/roi_moments_ref.box_catalogue), roi_mean0 [B, R] (the ROI means of the z = 0 volume, NaN for
the empty box), var_unit [B, R], cov_unit [B, P], abs_unit_var / abs_unit_cov (the sums of |d mean_r1/dz * d mean_r2/dz|: what the
tests' relative errors are taken to), voxel_factor [B] (the per-voxel variance factor at the one-voxel box, from unit latents as
tools/make_posterior_golden.py forms it).

Before writing, the generator asserts what the fixture is for: the whole-depth box has var_unit below 1e-24 of the largest, the pair
with disjoint footprints has covariance exactly 0, both covariance signs occur, and var_unit of the one-voxel box equals the
per-voxel factor there to 1e-12."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.make_golden import dump, fresh_process_state, import_reference, npy, sd_arrays  # noqa: E402
from roi_moments_ref import box_catalogue  # noqa: E402

D, H, W, B, S = 8, 12, 16, 2, 3
N_CH, COND_CH = 8, 4
PERTURB = 0.05          # as tools/make_posterior_golden.py: spreads s over several units


def main():
    import torch
    Ff, Fm, INN_utils, networks, unet, CWFA = import_reference()
    fresh_process_state(networks)
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(2626)
    torch.manual_seed(2600)
    np.random.seed(7)
    networks.networks_n_chans = N_CH
    arrs, inns, conds = {}, {}, {}
    for ix in (0, 1):
        Cn = D // 2 ** (ix + 1)
        _, built = networks.conditional_wavelet_flow(
            [D, H, W], [1, 29, H, W], networks.wavelet_flow_subnetwork2D,
            lambda: networks.cond_network(29, Cn, ix + 1, S, [], COND_CH),
            n_internal_ch=N_CH, n_down_steps=ix + 1, use_permutations=True, block_type="CAT", n_blocks=4)
        inn = built[ix].eval()
        with torch.no_grad():
            for p in inn.parameters():
                if p.requires_grad and p.dtype == torch.float32:
                    p.add_(torch.randn(p.shape, generator=g) * PERTURB)
        arrs.update(sd_arrays(inn, prefix=f"s{ix}/sd/"))
        for i, mdl in enumerate(inn.module_list):
            if type(mdl).__name__ == "PermuteDim":
                arrs[f"s{ix}/meta/axis_{i}"] = np.int64(mdl.dims_to_permute[1])
        c32 = [torch.randn(B, Cn, H, W, generator=g), 0.3 * torch.randn(B, Cn, H, W, generator=g)]
        arrs[f"s{ix}/c0"], arrs[f"s{ix}/c1"] = npy(c32[0]), npy(c32[1])
        inns[ix] = inn.double()
        for p in inns[ix].parameters():
            p.requires_grad_(False)
        conds[ix] = [t.double() for t in c32]
    low32 = torch.randn(B, D // 4, H, W, generator=g)
    low = low32.double()

    def pyramid(z1, z0):
        """z1: the coarser step's latent [B, 2, H, W]; z0: the finer step's [B, 4, H, W]."""
        mid, _ = inns[1]([z1, low], c=conds[1], rev=True)
        x, _ = inns[0]([z0, mid], c=conds[0], rev=True)
        return x

    boxes, pairs = box_catalogue(D, H, W)
    R, P = len(boxes), len(pairs)
    z1 = torch.zeros(B, D // 4, H, W, dtype=torch.float64, requires_grad=True)
    z0 = torch.zeros(B, D // 2, H, W, dtype=torch.float64, requires_grad=True)
    x = pyramid(z1, z0)
    assert tuple(x.shape) == (B, D, H, W)
    mean0 = np.full((B, R), np.nan)
    grads = {}
    for r, (a0, a1, y0, y1, x0, x1) in enumerate(boxes):
        if (a1 - a0) * (y1 - y0) * (x1 - x0) == 0:
            continue
        for b in range(B):
            m = x[b, a0:a1, y0:y1, x0:x1].mean()
            mean0[b, r] = float(m)
            g1, g0 = torch.autograd.grad(m, (z1, z0), retain_graph=True)
            other = 1 - b                                    # the samples of a batch do not mix
            assert not g1[other].any() and not g0[other].any()
            grads[b, r] = np.concatenate([npy(g1[b]).ravel(), npy(g0[b]).ravel()])
    var_unit, abs_var = np.full((B, R), np.nan), np.full((B, R), np.nan)
    cov_unit, abs_cov = np.full((B, P), np.nan), np.full((B, P), np.nan)
    for b in range(B):
        for r in range(R):
            if (b, r) in grads:
                var_unit[b, r] = abs_var[b, r] = float(grads[b, r] @ grads[b, r])
        for p, (r1, r2) in enumerate(pairs):
            if (b, r1) in grads and (b, r2) in grads:
                cov_unit[b, p] = float(grads[b, r1] @ grads[b, r2])
                abs_cov[b, p] = float(np.abs(grads[b, r1]) @ np.abs(grads[b, r2]))
    # --- the per-voxel factor at the one-voxel box, from unit latents
    with torch.no_grad():
        zz1, zz0 = torch.zeros_like(z1), torch.zeros_like(z0)
        x0v = pyramid(zz1, zz0)
        factor = (pyramid(torch.ones_like(zz1), zz0) - x0v) ** 2 + (pyramid(zz1, torch.ones_like(zz0)) - x0v) ** 2
    vz, vy, vx = boxes[0][0], boxes[0][2], boxes[0][4]
    voxel_factor = npy(factor[:, vz, vy, vx])
    # --- what the fixture is for
    largest = np.nanmax(var_unit)
    assert np.all(var_unit[:, 2] < 1e-24 * largest), f"whole-depth box: var_unit {var_unit[:, 2]} against {largest:.3e}"
    assert np.all(cov_unit[:, 2] == 0.0), f"disjoint footprints: covariance {cov_unit[:, 2]}"
    assert np.all(cov_unit[:, 0] > 0) and np.all(cov_unit[:, 1] < 0), f"covariance signs: {cov_unit[:, 0]}, {cov_unit[:, 1]}"
    assert np.all(np.isnan(cov_unit[:, 4])) and np.all(np.isnan(var_unit[:, 4]))
    rel = np.abs(var_unit[:, 0] / voxel_factor - 1.0).max()
    assert rel < 1e-12, f"one-voxel box against the per-voxel factor: {rel:.3e}"
    print(f"var_unit: {np.nanmin(var_unit[:, [0, 1, 3, 5, 6, 7, 8, 9, 10]]):.4e} .. {largest:.4e}; cov_unit(+) {cov_unit[:, 0]}, (-) {cov_unit[:, 1]}; "
          f"one voxel vs per-voxel factor {rel:.2e}")
    arrs.update(low=npy(low32), boxes=boxes, pairs=pairs, roi_mean0=mean0, var_unit=var_unit, cov_unit=cov_unit, abs_unit_var=abs_var,
                abs_unit_cov=abs_cov, voxel_factor=voxel_factor, D=np.int64(D), H=np.int64(H), W=np.int64(W), n_ch=np.int64(N_CH),
                cond_ch=np.int64(COND_CH))
    dump("g26_roi_moments", **arrs)


if __name__ == "__main__":
    main()
