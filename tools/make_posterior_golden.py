"""Write the posterior fixture tests/golden/g24_posterior.npz: one CAT step built by the REFERENCE's own conditional_wavelet_flow
(imported by oracle.make_golden's recipe; small channel counts as tests/test_host_logic.build_step: n_ch = 8, cond_ch = 4;
D = 6, H = 24, W = 64, B = 2, step index 0, so C = 3 detail channels), cast to float64, with seeded conditions and low band, and what
the step's inverse returns for them.  State dict, inputs and outputs only.  Run from the repository root:
    python tools/make_posterior_golden.py

The reference's own temperature != 0 path raises a NameError, so the reference fixes the MAP (weights -> coefficients -> volume) and
the moments follow from that map: in a CAT step every s,t depends on the conditions only, so x = step([z, low], c, rev=True) is
elementwise-affine in z and
    x0         = step([0, low])                    the posterior mean (E z = 0)
    var_factor = (step([1, low]) - x0)^2           the per-voxel variance for unit-variance latents.

Arrays: sd/* (the state dict, fp32 as built: the float64 cast of an fp32 value is exact), meta/axis_i (PermuteDim axes, not part of
the state dict), c0, c1, low (fp32 as drawn; the step runs on their float64 casts), x0, var_factor (float64), var_factor_min,
var_factor_max.

Before writing, the generator asserts what the fixture is for: the step is elementwise-affine (for three random z,
step([z, low]) - x0 equals (step([1, low]) - x0) times z pulled through the step's permutations), var_factor spans more than two
decades, and the two planes of every depth pair agree."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import dump, fresh_process_state, import_reference, npy, sd_arrays  # noqa: E402

D, H, W, B, IX, S = 6, 24, 64, 2, 0, 3
N_CH, COND_CH = 8, 4
PERTURB = 0.05          # added to every parameter (the `_first` sub-network's last conv starts near zero): spreads s over several units


def main():
    import torch
    Ff, Fm, INN_utils, networks, unet, CWFA = import_reference()
    fresh_process_state(networks)
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(2424)
    torch.manual_seed(2400)
    np.random.seed(7)
    networks.networks_n_chans = N_CH                     # (as oracle.make_golden's step fixtures set it)
    Cn = D // 2 ** (IX + 1)
    assert Cn == 3
    cond_net, inns = networks.conditional_wavelet_flow(
        [D, H, W], [1, 29, H, W], networks.wavelet_flow_subnetwork2D,
        lambda: networks.cond_network(29, Cn, IX + 1, S, [], COND_CH),
        n_internal_ch=N_CH, n_down_steps=IX + 1, use_permutations=True, block_type="CAT", n_blocks=4)
    inn = inns[IX].eval()
    for p in inn.parameters():
        if p.requires_grad and p.dtype == torch.float32:
            p.add_(torch.randn(p.shape, generator=g) * PERTURB)
    arrs = sd_arrays(inn)                                # fp32, before the cast
    perms = []                                           # (inverse table, axis) in graph order
    for i, mdl in enumerate(inn.module_list):
        cls = type(mdl).__name__
        if cls == "PermuteDim":
            arrs[f"meta/axis_{i}"] = np.int64(mdl.dims_to_permute[1])
            perms.append((mdl.perm_inv.clone(), int(mdl.dims_to_permute[1])))
        elif cls == "PermuteRandom":
            perms.append((mdl.perm_inv.clone(), 1))
    inn = inn.double()
    c32 = [torch.randn(B, Cn, H, W, generator=g), 0.3 * torch.randn(B, Cn, H, W, generator=g)]
    low32 = torch.randn(B, Cn, H, W, generator=g)
    c, low = [t.double() for t in c32], low32.double()

    def step(z):
        x, _ = inn([z, low], c=c, rev=True)
        return x

    zeros = torch.zeros(B, Cn, H, W, dtype=torch.float64)
    x0 = step(zeros)
    gain = step(torch.ones_like(zeros)) - x0             # signed: +e/sqrt2 on the even plane, -e/sqrt2 on the odd one
    var_factor = gain ** 2
    # --- the step is elementwise-affine in z: x - x0 = gain * (z pulled through the inverse's gathers, applied last-module-first)
    for _ in range(3):
        z = torch.randn(B, Cn, H, W, generator=g, dtype=torch.float64)
        zp = z
        for table, axis in reversed(perms):
            zp = zp.index_select(axis, table.to(torch.long))
        want = gain * zp.repeat_interleave(2, dim=1)
        got = step(z) - x0
        err = float((got - want).abs().max() / want.abs().max())
        assert err < 1e-12, f"the step is not elementwise-affine in z: {err:.3e}"
    vmin, vmax = float(var_factor.min()), float(var_factor.max())
    assert vmin > 0 and vmax / vmin > 100.0, f"var_factor spans only {vmax / vmin:.1f}x"
    pair = float(((var_factor[:, 0::2] - var_factor[:, 1::2]).abs() / var_factor[:, 0::2]).max())
    # equal up to the rounding of (low +- v1) - (low +- v0): a few 2^-53 * |x0| / |gain|, twice that after squaring (|x0| / |gain| reaches 1e4)
    assert pair < 1e-10, f"the two planes of a depth pair differ by {pair:.3e}"
    print(f"var_factor: min {vmin:.4e}, max {vmax:.4e} ({np.log10(vmax / vmin):.2f} decades)")
    arrs.update(c0=npy(c32[0]), c1=npy(c32[1]), low=npy(low32), x0=npy(x0), var_factor=npy(var_factor),
                var_factor_min=np.float64(vmin), var_factor_max=np.float64(vmax),
                D=np.int64(D), H=np.int64(H), W=np.int64(W), ix=np.int64(IX), n_ch=np.int64(N_CH), cond_ch=np.int64(COND_CH))
    dump("g24_posterior", **arrs)


if __name__ == "__main__":
    main()
