"""Write the evaluation fixtures tests/golden/g21_eval_*.npz: seeded inputs, arguments and the outputs of the REFERENCE's own
compute_INN_step_performance, volume_2_projections and corr_coeff_3D on the CPU (imported by oracle.make_golden's recipe).
Inputs, arguments and outputs only.  Run from the repository root:  python tools/make_eval_golden.py

The generator asserts the gate conditions the tests rely on (a discrete gate must not be able to hide a difference): no
masked-MAE element on the threshold; every in-volume ROI of the first corr_coeff_3D case passes the range gate in the first
sweep; the dim case enters the halving loop exactly once; no ROI range within 1e-3 relative of a gate threshold."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.make_golden import dump, import_reference  # noqa: E402

import eval_ref as R  # noqa: E402


def npy(t):
    return t.detach().cpu().numpy()


def main():
    import torch
    CWFA = import_reference()[-1]
    import utils as RU                                   # the reference's utils (import_reference put it on the path)
    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(2121)

    # ------------------------------------------------------------------ step metrics
    gt = torch.randn(1, 16, 24, 28, generator=g) * 0.7 + 0.2
    pred = gt + torch.randn(1, 16, 24, 28, generator=g) * 0.15
    mean, std = 0.31, 1.7
    arrs = dict(gt=npy(gt), pred=npy(pred), mean=np.float32(mean), std=np.float32(std))
    cases = []
    for step in (0, 2):
        for norm in (False, True):
            for ths in (0.05, 0.0):
                name = f"s{step}_n{int(norm)}_t{int(ths != 0)}"
                try:
                    p, m, graw, praw = CWFA.compute_INN_step_performance(gt.clone(), pred.clone(), step, mean, std, norm, ths)
                    raised = 0
                    thr = praw.abs().max() * ths
                    assert int((praw == thr).sum()) == 0, "a masked-MAE element lies on the threshold"
                except UnboundLocalError:                # ths == 0: the reference never assigns masked_psnr
                    p, m, raised = float("nan"), float("nan"), 1
                cases.append(name)
                arrs[name + "/psnr"], arrs[name + "/mape"], arrs[name + "/raised"] = np.float64(p), np.float64(m), np.int64(raised)
                if not raised and ths != 0 and (step, norm) in ((0, False), (2, True)):
                    arrs[name + "/gt_raw"], arrs[name + "/pred_raw"] = npy(graw), npy(praw)
    # the two mse == 0 branches of psnr
    same = torch.randn(1, 4, 6, 8, generator=g)
    arrs["same"] = npy(same)
    p, m, _, _ = CWFA.compute_INN_step_performance(same.clone(), same.clone(), 1, mean, std)
    arrs["same/psnr"], arrs["same/mape"] = np.float64(p), np.float64(m)
    zero = torch.zeros(1, 4, 6, 8)
    p, m, _, _ = CWFA.compute_INN_step_performance(zero.clone(), zero.clone(), 1, 0.0, std)
    arrs["zero/psnr"], arrs["zero/mape"] = np.float64(p), np.float64(m)
    assert arrs["same/psnr"] == 100 and arrs["zero/psnr"] == 0
    arrs["cases"] = np.array(cases)
    dump("g21_eval_metrics", **arrs)

    # ------------------------------------------------------------------ projections
    v = torch.randn(2, 12, 20, 20, generator=g)
    v5 = v.permute(0, 2, 3, 1).unsqueeze(1)
    arrs = dict(vol=npy(v))
    calls = {"default": {}, "depths_in_ch": dict(depths_in_ch=True), "normalize": dict(normalize=True),
             "ths": dict(ths=[0.1, 0.9]), "normalize_ths": dict(normalize=True, ths=[0.1, 0.9]), "bars": dict(add_scale_bars=True),
             "scale3_border3": dict(scaling_factors=[1, 1, 3], border_thickness=3),
             "all": dict(normalize=True, ths=[0.2, 0.7], add_scale_bars=True, scaling_factors=[1, 1, 4], border_thickness=1)}
    for name, kw in calls.items():
        if kw.get("depths_in_ch"):
            out = RU.volume_2_projections(v.clone(), **kw)
        else:
            out = RU.volume_2_projections(v5.clone(), **kw)
        arrs["out/" + name] = npy(out)
    vn = torch.randn(1, 12, 20, 24, generator=g)                        # H != W: the reference's composite does not exist
    arrs["vol_nonsquare"] = npy(vn)
    try:
        RU.volume_2_projections(vn.permute(0, 2, 3, 1).unsqueeze(1))
        arrs["nonsquare_raised"] = np.int64(0)
    except RuntimeError:
        arrs["nonsquare_raised"] = np.int64(1)
    try:                                                                # a scaled plane: the unscaled image does not fit its slot
        RU.volume_2_projections(v5.clone(), scaling_factors=[2, 1, 2])
        arrs["scaled_plane_raised"] = np.int64(0)
    except RuntimeError:
        arrs["scaled_plane_raised"] = np.int64(1)
    dump("g21_eval_projections", **arrs)

    # ------------------------------------------------------------------ corr_coeff_3D
    T, D, H, W, r12, r3 = 24, 32, 40, 40, 5, 3
    # (x, y, z): z counts from the central planes (shift D//2 - 13 = 3).  Boxes clipped at every face, one outside in depth.
    coords = [(20, 20, 12), (2, 20, 12), (38, 10, 12), (20, 2, 12), (10, 38, 12), (20, 30, -2), (30, 20, 27), (8, 8, 10), (32, 32, 14),
              (8, 30, 20), (30, 8, 6), (20, 10, 40)]
    boxes = R.roi_boxes(coords, (T, D, H, W), r12, r3)
    assert (boxes[-1, 1] - boxes[-1, 0]) == 0 and all(boxes[:-1, 1] > boxes[:-1, 0])
    t = np.arange(T)
    n = len(coords)
    wave = np.stack([0.5 + 0.5 * np.sin(2 * np.pi * t / (8 + i) + i) for i in range(n)])
    other = np.stack([0.5 + 0.5 * np.sin(2 * np.pi * t / (5 + i) + 2 * i) for i in range(n)])
    same_period = np.stack([0.5 + 0.5 * np.sin(2 * np.pi * t / 12 + i) for i in range(n)])
    for case, amp, bg in (("bright", np.ones(n), 0.002), ("dim", np.r_[1.0, 0.45 * np.ones(n - 1)], None)):
        base_wave = wave if case == "bright" else same_period
        act_gt = (amp[:, None] * base_wave).astype(np.float32)
        act_pred = (amp[:, None] * (0.8 * base_wave + 0.25 * other)).astype(np.float32)
        for fw in (10, 0):
            if case == "dim":
                # background so that median * 50 lies between the strong ROI's range and the weak ones', and half of it below all
                st0 = R.make_stack(7, T, (D, H, W), boxes, act_gt, 1e-4, 1e-4)
                peak = float(st0.max())
                rng = np.sort([R.norm_data(r, min(fw, 6) if fw else 0)[1] for r in R.roi_means(st0, boxes)[:-1]]) / peak
                target = 1.25 * rng[-2]                                               # between the weak ranges and the strong one
                assert target < 0.8 * rng[-1], rng
                assert target / 2 < 0.9 * rng[0], rng
                bg = target / 50 * peak / 0.625                                       # median of U(0, bg) + U(0, bg / 4)
            sg = R.make_stack(7, T, (D, H, W), boxes, act_gt, bg, bg / 4)
            sp = R.make_stack(8, T, (D, H, W), boxes, act_pred, bg, bg / 4)
            seen = []
            real_meshgrid = np.meshgrid

            def spy(xpix, ypix, zpix):
                seen.append([(a[0], a[-1] + 1) if len(a) else (0, 0) for a in (zpix, ypix, xpix)])
                return real_meshgrid(xpix, ypix, zpix)
            np.meshgrid = spy
            try:
                ccs, df = CWFA.corr_coeff_3D(torch.from_numpy(sg.copy()), torch.from_numpy(sp.copy()), [list(c) for c in coords], r12, r3,
                                             filter_width=fw)
            finally:
                np.meshgrid = real_meshgrid
            ranges = np.array(seen[:n]).reshape(n, 6)
            # gate conditions, on the reference's own results
            norm_g = torch.from_numpy(sg) / float(sg.max())
            img_ths = float(norm_g[norm_g > 0].median()) * 50
            tr = R.roi_means(norm_g.numpy(), boxes)[:-1]
            rr = np.array([R.norm_data(r, min(fw, 6) if fw else 0)[1] for r in tr])
            sweeps = 1 if case == "bright" else 2
            for k in range(sweeps):
                assert np.all(np.abs(rr / (img_ths / 2 ** k) - 1) > 1e-3), "a ROI range within 1e-3 of the gate"
            if case == "bright":
                assert np.all(rr > img_ths) and len(ccs) == n, (rr, img_ths, len(ccs))
            else:
                assert (rr > img_ths).sum() == 1 and np.all(rr > img_ths / 2) and len(ccs) == 2 + n, (rr, img_ths, len(ccs))
            dump(f"g21_eval_corr_{case}_fw{fw}", coords=np.array(coords, dtype=np.int64), boxes=ranges.astype(np.int32), act_gt=act_gt,
                 act_pred=act_pred, bg=np.float64(bg), seeds=np.array([7, 8]), shape=np.array([T, D, H, W]), r12=np.int64(r12), r3=np.int64(r3),
                 filter_width=np.int64(fw), checksum=np.array([sg.astype(np.float64).sum(), sp.astype(np.float64).sum()]),
                 ccs=np.array(ccs, dtype=np.float64), df_values=df.to_numpy(dtype=np.float64), df_index=np.array(df.index, dtype=np.int64),
                 df_columns=np.array(list(df.columns)), n_sweeps=np.int64(sweeps))


if __name__ == "__main__":
    main()
