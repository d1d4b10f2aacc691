"""GPU: the evaluation pass on the MI355X -- every mirror against the reference's recorded results (tests/golden/g21_eval_*.npz),
every kernel against the float64 restatement (tests/eval_ref.py) on ragged and full sizes, and everything twice, bitwise equal.

Bounds.  Bit-exact: raw volumes, extrema, projections, composites, medians, index ranges (max and selection are independent of
the order; the element-wise steps are the reference's fp32 operations).  1e-8 relative against the float64 restatement for the
device sums: float64 accumulations of at most 2^25 fp32 terms, worst case N * 2^-53 = 4e-9; the masked count exact.  1e-4 against
the reference's own values (it sums in fp32 in torch's / numpy's orders): conftest.assert_close, the project's bound."""
import numpy as np
import pytest
import torch
from conftest import assert_close, load_golden

import eval_ref as R
from test_eval_cpu import CORR, PROJ, assert_frame, metric_cases, stacks_of

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def npy(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(np.atleast_1d(np.asarray(a))), np.ascontiguousarray(np.atleast_1d(np.asarray(b)))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def twice(fn):
    """Run fn twice; every tensor / array / number of the two results must agree bit for bit.  Returns the first result."""
    r1, r2 = fn(), fn()
    f1 = r1 if isinstance(r1, (tuple, list)) else (r1,)
    f2 = r2 if isinstance(r2, (tuple, list)) else (r2,)
    for u, v in zip(f1, f2):
        if torch.is_tensor(u):
            assert same_bits(npy(u), npy(v)), "two runs differ"
        elif hasattr(u, "columns"):
            assert list(u.columns) == list(v.columns) and list(u.index) == list(v.index), "two runs differ"
            assert same_bits(u.to_numpy(dtype=np.float64), v.to_numpy(dtype=np.float64)), "two runs differ"
        elif u is not None:
            assert same_bits(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)), "two runs differ"
    return r1


def volumes(shape, seed, views=False):
    """(pred, gt) device tensors of `shape` and their numpy values; views: channel slices of a larger tensor with a batch stride."""
    rs = np.random.RandomState(seed)
    B, D, H, W = shape
    g = (rs.standard_normal(shape) * 0.7 + 0.2).astype(np.float32)
    p = (g + rs.standard_normal(shape) * 0.15).astype(np.float32)
    if not views:
        return dev(p), dev(g), p, g
    big_p, big_g = torch.zeros(B, D + 3, H, W, device="cuda"), torch.zeros(B, D + 5, H, W, device="cuda")
    big_p[:, 1:D + 1], big_g[:, 2:D + 2] = dev(p), dev(g)
    return big_p[:, 1:D + 1], big_g[:, 2:D + 2], p, g


RAGGED = [((1, 5, 7, 9), False), ((1, 7, 9, 131), False), ((1, 1, 6, 10), False), ((3, 4, 8, 8), True), ((2, 6, 33, 33), True), ((1, 3, 20, 258), False),
          ((1, 9, 18, 516), False)]
LEVELS = [(1, 96 // 2 ** n, 512, 512) for n in range(5)]


# ------------------------------------------------------------------------------------------------ mirrors vs the fixtures
def test_step_performance_matches_reference():
    from cwfa_amd import CWFA
    fx = load_golden("g21_eval_metrics")
    gt, pred, mean, std = dev(fx["gt"]), dev(fx["pred"]), float(fx["mean"]), float(fx["std"])
    for name, step, norm, ths in metric_cases(fx):
        p, m, graw, praw = twice(lambda: CWFA.compute_INN_step_performance(gt, pred, step, mean, std, norm, ths))
        ep, em, eg, epr = R.step_performance(fx["gt"], fx["pred"], step, fx["mean"], fx["std"], norm, ths)
        assert same_bits(npy(graw), eg) and same_bits(npy(praw), epr), name
        assert abs(p - ep) <= 1e-8 * abs(ep) and abs(m - em) <= 1e-8 * abs(em), (name, p, ep, m, em)
        print(f"{name}: psnr {p:.9f} (restatement rel {abs(p - ep) / abs(ep):.1e}) mape {m:.9f} ({abs(m - em) / abs(em):.1e})")
        if not int(fx[name + "/raised"]):
            rp, rm = float(fx[name + "/psnr"]), float(fx[name + "/mape"])
            print(f"   vs reference: psnr rel {abs(p - rp) / abs(rp):.2e}, mape rel {abs(m - rm) / abs(rm):.2e}")
            assert abs(p - rp) <= 1e-4 * abs(rp) and abs(m - rm) <= 1e-4 * abs(rm), name
            if name + "/gt_raw" in fx:
                assert same_bits(npy(graw), fx[name + "/gt_raw"]) and same_bits(npy(praw), fx[name + "/pred_raw"]), name
        # the fused form gives the same scalars without the raw volumes (no normaliaze_before_metrics there)
        if not norm:
            fp, fm = CWFA.evaluate_step(gt, pred, step, mean, std, ths, projections=False)[:2]
            assert fp == p and fm == m, name
    same, zero = dev(fx["same"]), torch.zeros(1, 4, 6, 8, device="cuda")
    p, m = CWFA.compute_INN_step_performance(same, same, 1, mean, std)[:2]
    assert p == 100.0 == float(fx["same/psnr"]) and abs(m - float(fx["same/mape"])) <= 1e-4 * float(fx["same/mape"])
    assert CWFA.compute_INN_step_performance(zero, zero, 1, 0.0, std)[:2] == (0.0, 0.0)


def test_psnr_mirror():
    from cwfa_amd import utils
    fx = load_golden("g21_eval_metrics")
    a, b = dev(fx["gt"]), dev(fx["pred"])
    got = twice(lambda: utils.psnr(a, b))
    want = R.psnr_from(R.metric_sums(fx["pred"], fx["gt"])[0, 0], 1.0, fx["gt"].size)
    assert got.dtype == torch.float32 and abs(float(got) - want) <= 1e-6 * abs(want)
    assert abs(float(utils.psnr(a, b, PIXEL_MAX=2.0)) - R.psnr_from(R.metric_sums(fx["pred"], fx["gt"])[0, 0], 1.0, fx["gt"].size, 2.0)) < 1e-5
    z = torch.zeros(2, 3, device="cuda")
    assert utils.psnr(a, a).tolist() == [100] and utils.psnr(z, z).tolist() == [0]


@pytest.mark.parametrize("name", sorted(PROJ))
def test_volume_2_projections_matches_reference(name):
    from cwfa_amd import utils
    fx = load_golden("g21_eval_projections")
    v = dev(fx["vol"])
    kw = dict(PROJ[name])
    args = dict(normalize=kw.get("normalize", False), ths=list(kw.get("ths", (0.0, 1.0))), add_scale_bars=kw.get("bars", False),
                scaling_factors=[1, 1, kw.get("depth_scale", 2)], border_thickness=kw.get("border", 2))
    if name == "depths_in_ch":
        out = twice(lambda: utils.volume_2_projections(v, depths_in_ch=True, **args))
    else:
        out = twice(lambda: utils.volume_2_projections(v.permute(0, 2, 3, 1).unsqueeze(1), **args))
    assert not out.is_cuda and same_bits(npy(out), fx["out/" + name])
    on = utils.volume_2_projections(v, depths_in_ch=True, on_device=True, **args)
    assert on.is_cuda and same_bits(npy(on), fx["out/" + name])


def test_volume_2_projections_rejects_what_the_reference_cannot_compose():
    from cwfa_amd import utils
    fx = load_golden("g21_eval_projections")
    assert int(fx["nonsquare_raised"]) == 1 and int(fx["scaled_plane_raised"]) == 1
    with pytest.raises(ValueError, match="H = 20 != W = 24"):
        utils.volume_2_projections(dev(fx["vol_nonsquare"]), depths_in_ch=True)
    with pytest.raises(ValueError, match="scaling_factors"):
        utils.volume_2_projections(dev(fx["vol"]), depths_in_ch=True, scaling_factors=[2, 1, 2])
    with pytest.raises(NotImplementedError, match="permuted view"):
        utils.volume_2_projections(dev(fx["vol"]).permute(0, 2, 3, 1).unsqueeze(1).contiguous())


@pytest.mark.parametrize("name", CORR)
def test_corr_coeff_3D_matches_reference(name):
    from cwfa_amd import CWFA
    fx = load_golden(name)
    sg, sp = stacks_of(fx)
    dg, dp = dev(sg), dev(sp)
    coords = [tuple(int(v) for v in c) for c in fx["coords"]]
    ccs, df = twice(lambda: CWFA.corr_coeff_3D(dg, dp, coords, int(fx["r12"]), int(fx["r3"]), filter_width=int(fx["filter_width"])))
    assert same_bits(npy(dg), sg) and same_bits(npy(dp), sp), "corr_coeff_3D changed its inputs"
    assert list(df.columns) == [str(c) for c in fx["df_columns"]] and list(df.index) == list(fx["df_index"])
    vals = df.to_numpy(dtype=np.float64)
    assert len(ccs) == len(fx["ccs"]) and np.array_equal(np.isnan(vals), np.isnan(fx["df_values"]))
    print(f"{name}: cc max abs diff {np.nanmax(np.abs(np.array(ccs, dtype=np.float64) - fx['ccs'])):.2e}, "
          f"frame max abs diff {np.nanmax(np.abs(vals - fx['df_values'])):.2e}")
    assert_close(np.nan_to_num(np.array(ccs, dtype=np.float64)), np.nan_to_num(fx["ccs"]), what="correlation coefficients")
    assert_frame(vals, fx["df_values"])
    print(f"   traces alone: max abs diff {np.nanmax(np.abs(vals[:, 6:] - fx['df_values'][:, 6:])):.2e}")
    # the device reductions behind it: traces to 1e-8, the median bit-exact
    from cwfa_amd import ops
    tr = npy(ops.roi_means(dg, fx["boxes"]))
    want = R.roi_means(sg, fx["boxes"])
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(tr), np.isnan(want)) and rel(tr[ok], want[ok]) <= 1e-8
    med, cnt = ops.select_positive(dg)
    ref_med = torch.from_numpy(sg)[torch.from_numpy(sg) > 0].median()
    assert same_bits(npy(med)[0], ref_med.numpy()) and int(cnt) == int((sg > 0).sum())
    assert same_bits(np.float32(npy(med)[0]) / sg.max(), (torch.from_numpy(sg / sg.max())[torch.from_numpy(sg) > 0]).median().numpy())


# ------------------------------------------------------------------------------------------------ kernels vs the restatement
def check_kernels(shape, views, seed, affine=True):
    from cwfa_amd import ops
    pred, gt, p, g = volumes(shape, seed, views)
    step, mean, std = 2, 0.31, 1.7
    aff = ops.eval_affine(step, mean, std) if affine else None
    pr, gr = (R.raw_volume(p, step, mean, std), R.raw_volume(g, step, mean, std)) if affine else (p, g)
    ext = npy(twice(lambda: ops.volume_extrema(pred, gt, aff)))
    assert same_bits(ext, R.extrema(pr, gr)), "extrema"
    assert same_bits(npy(ops.volume_extrema(pred, None, aff))[:, :4], R.extrema(pr)[:, :4])
    thr = float(np.float32(ext[:, 3].max()) * np.float32(0.05))
    off_p, off_g = float(ext[:, 0].min()), float(ext[:, 4].min())
    for kw, (a, b) in (({}, (pr, gr)), (dict(pred_offset=off_p, gt_offset=off_g), (pr - np.float32(off_p), gr - np.float32(off_g)))):
        sums = npy(twice(lambda: ops.volume_metrics(pred, gt, thr, aff, **kw)))
        want = R.metric_sums(a, b, thr)
        assert np.array_equal(sums[:, 3], want[:, 3]), "masked count"
        worst = rel(sums[:, :3], want[:, :3])
        assert worst <= 1e-8, f"metric sums: {worst:.2e}"
    worst_all = worst
    zs = twice(lambda: ops.mip3(pred, gt, triple=True, affine=aff))
    for q, v in enumerate((np.abs(pr), np.abs(gr), np.abs(pr - gr))):
        for got, ref in zip(zs, R.mip3(v)):
            assert same_bits(npy(got[q]), np.ascontiguousarray(ref)), f"projection set {q}"
    for a_, b_, v in ((pred, None, np.abs(pr)), (pred, gt, np.abs(pr - gr))):
        for got, ref in zip(twice(lambda: ops.mip3(a_, b_, affine=aff)), R.mip3(v)):
            assert same_bits(npy(got), np.ascontiguousarray(ref)), "single projection"
    k = p.size // 3
    val, cnt = twice(lambda: ops.select_positive(pred, k))
    pos = torch.sort(torch.from_numpy(p)[torch.from_numpy(p) > 0]).values
    assert int(cnt) == len(pos) and (same_bits(npy(val)[0], pos[k].numpy()) if k < len(pos) else bool(torch.isnan(val).all()))
    med, _ = ops.select_positive(pred)
    assert same_bits(npy(med)[0], torch.from_numpy(p)[torch.from_numpy(p) > 0].median().numpy())
    return worst_all


@pytest.mark.parametrize("shape,views", RAGGED)
def test_kernels_ragged(shape, views):
    check_kernels(shape, views, seed=sum(shape))
    check_kernels(shape, views, seed=1 + sum(shape), affine=False)


@pytest.mark.parametrize("shape", LEVELS)
def test_kernels_full_size_levels(shape):
    worst = check_kernels(shape, False, seed=shape[1])
    print(f"{shape}: worst relative error of the float64 sums {worst:.2e}")


def test_projection_maps_in_kernel_vs_restatement():
    """normalize / thresholds applied on load, on a ragged square volume, against the fp32 restatement, bit for bit."""
    from cwfa_amd import utils
    rs = np.random.RandomState(5)
    v = rs.standard_normal((2, 7, 37, 37)).astype(np.float32)
    for kw in (dict(normalize=True), dict(ths=(0.3, 0.6)), dict(normalize=True, ths=(0.05, 0.95), bars=True, depth_scale=3, border=0)):
        out = twice(lambda: utils.volume_2_projections(dev(v), depths_in_ch=True, normalize=kw.get("normalize", False),
                                                       ths=list(kw.get("ths", (0.0, 1.0))), add_scale_bars=kw.get("bars", False),
                                                       scaling_factors=[1, 1, kw.get("depth_scale", 2)], border_thickness=kw.get("border", 2)))
        assert same_bits(npy(out), R.projections(v, **kw)), kw


@pytest.mark.parametrize("shape", [(1, 12, 64, 64), (1, 96, 512, 512)])
def test_evaluate_step_is_the_loop_body(shape):
    """evaluate_step == compute_INN_step_performance + three volume_2_projections calls on its raw volumes (CWFA.py:1073-1085)."""
    from cwfa_amd import CWFA, utils
    pred, gt, p, g = volumes(shape, 11)
    step, mean, std = 1, 0.2, 1.3
    fp, fm, ip, ig, idf = twice(lambda: CWFA.evaluate_step(gt, pred, step, mean, std))
    cp, cm, graw, praw = CWFA.compute_INN_step_performance(gt, pred, step, mean, std)
    assert fp == cp and fm == cm
    pr, gr = R.raw_volume(p, step, mean, std), R.raw_volume(g, step, mean, std)
    diff = dev(np.abs(pr - gr))
    for img, vol in ((ip, praw), (ig, graw), (idf, diff)):
        assert same_bits(npy(img), npy(utils.volume_2_projections(vol.permute(0, 2, 3, 1).unsqueeze(1))))
    assert same_bits(npy(ip), R.projections(pr)) and same_bits(npy(idf), R.projections(np.abs(pr - gr)))
    ep, em, _, _ = R.step_performance(g, p, step, mean, std)
    assert abs(fp - ep) <= 1e-8 * abs(ep) and abs(fm - em) <= 1e-8 * abs(em)


def test_select_positive_corner_cases():
    from cwfa_amd import ops

    def run(x, k):
        val, cnt = twice(lambda: ops.select_positive(dev(x.reshape(1, 1, 1, -1)), k))
        return npy(val)[0], int(cnt)

    rs = np.random.RandomState(3)
    dup = rs.randint(-3, 6, size=4099).astype(np.float32) * np.float32(0.37)                      # many duplicates, negatives, zeros
    tiny = np.concatenate([np.arange(1, 40, dtype=np.uint32).view(np.float32), np.float32([1e-30, 3.0, -1.0, 0.0])])   # denormals
    for x in (dup, tiny, np.full(1000, 2.5, dtype=np.float32), np.float32([-1.0, 0.0, 7.25, -0.0]), rs.standard_normal(70001).astype(np.float32)):
        pos = torch.sort(torch.from_numpy(x)[torch.from_numpy(x) > 0]).values.numpy()
        for k in (0, len(pos) - 1, len(pos) // 2, -1):
            val, cnt = run(x, k)
            want = pos[k] if k >= 0 else torch.from_numpy(pos).median().numpy()
            assert cnt == len(pos) and same_bits(val, want), (k, val, want)
        if len(pos) < len(x):
            val, cnt = run(x, len(pos))                                                              # k >= count: NaN
            assert cnt == len(pos) and np.isnan(val)
    val, cnt = run(np.float32([-1.0, 0.0, -2.0]), -1)
    assert cnt == 0 and np.isnan(val)


def test_roi_means_many_boxes_and_views():
    from cwfa_amd import ops
    rs = np.random.RandomState(9)
    T, D, H, W = 5, 9, 21, 23
    st = rs.standard_normal((T, D, H, W)).astype(np.float32)
    big = torch.zeros(T, D + 4, H, W, device="cuda")
    big[:, 2:D + 2] = dev(st)
    lo = np.stack([rs.randint(0, n, size=300) for n in (D, H, W)], 1)
    hi = np.minimum(lo + np.stack([rs.randint(0, 7, size=300) for _ in range(3)], 1), [D, H, W])
    boxes = np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1], lo[:, 2], hi[:, 2]], 1).astype(np.int32)
    got = npy(twice(lambda: ops.roi_means(big[:, 2:D + 2], boxes)))
    want = R.roi_means(st, boxes)
    assert np.isnan(want).any() and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-3))) <= 1e-8
    with pytest.raises(RuntimeError, match="not inside"):
        ops.roi_means(dev(st), [[0, D + 1, 0, 1, 0, 1]])


def test_mirrors_under_autocast():
    from cwfa_amd import CWFA, utils
    fx = load_golden("g21_eval_projections")
    v = dev(fx["vol"])
    with torch.autocast("cuda", dtype=torch.float16):
        out = utils.volume_2_projections(v, depths_in_ch=True)
        p, m = CWFA.evaluate_step(v, v * 0.5, 0, 0.0, 1.0, projections=False)[:2]
    assert same_bits(npy(out), fx["out/default"]) and np.isfinite(p) and np.isfinite(m)
