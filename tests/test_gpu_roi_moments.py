"""GPU (MI355X): the exact ROI-mean moments of a CAT pyramid -- cwfa_chain_inv_roi_cov_f32 against the float64
restatement tests/roi_moments_ref.py on the same fp32 inputs, its exact cases bit for bit, CWFA.posterior_roi_moments against the
per-voxel route, against the reference fixture g26_roi_moments and against the seeded sampler.

Bounds.  The error of a pair is relative to the SUM OF THE ABSOLUTE TERMS of that pair.  The launch adds the same s values in the same
order and takes the same expf as chain_inv_var_kernel; on top come integer weights and a double sum, so the kernel is held to
VAR_BOUND of tests/test_gpu_posterior.py and the fixture cases, which add the sub-networks' arithmetic, to its FIX_BOUND.  The
statistical bounds are derived in the test's docstring, not measured."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, sd_of

import roi_moments_ref as M
from test_gpu_posterior import FIX_BOUND, TOL, VAR_BOUND, _pyramid

pytestmark = pytest.mark.gpu

Z1 = 0.29112509477279314     # z_var(T = 1)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


def ref_chain(shape, axes, seed, no_s=(), no_t=(), kinds=None, pres=None, clamps=None):
    """posterior_ref stage dicts from seeded fp32 draws; the last stage is the pass-through one (t := -t / sqrt 2)."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    ref = []
    for k, ax in enumerate(axes):
        ref.append({"s_raw": None if k in no_s else torch.randn(shape, generator=g),
                    "t": None if k in no_t else torch.randn(shape, generator=g),
                    "perm": None if ax is None else torch.randperm([0, C, H, W][ax], generator=g), "axis": ax,
                    "kind": kinds[k] if kinds else "ATAN", "clamp": clamps[k] if clamps else 2.0, "pre": pres[k] if pres else 1.0,
                    "neg": k == len(axes) - 1})
    return ref


def dev_chain(ref, with_t=True):
    from cwfa_amd import ops
    out = []
    for st in ref:
        out.append(ops.stage(None if st["s_raw"] is None else st["s_raw"].cuda(), st["t"].cuda() if with_t and st["t"] is not None else None,
                             st["kind"], st["clamp"], pre_scale=st["pre"], t_neg_div_sqrt2=st["neg"],
                             perm=None if st["perm"] is None else st["perm"].cuda(), axis=st["axis"] or 1))
    return out


def all_pairs(boxes, pairs):
    return np.concatenate([np.repeat(np.arange(len(boxes), dtype=np.int32)[:, None], 2, 1), pairs])


def run(dev, z_var, shape, m, boxes, pairs=None, out=None):
    from cwfa_amd import ops
    if out is None:
        P = boxes.n_pairs if isinstance(boxes, ops.RoiPairs) else len(boxes) if pairs is None else len(pairs)
        out = torch.zeros(shape[0], P, dtype=torch.float64, device="cuda")
    return ops.chain_inv_roi_cov(out, dev, z_var, shape, m, boxes, pairs)


def rel_to_terms(got, want, mag):
    """max |got - want| / mag over the pairs with terms; NaN exactly where want is NaN, and EXACT zeros where there are no terms."""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    live = ~np.isnan(want) & (mag > 0)
    dead = ~np.isnan(want) & (mag == 0)
    assert np.all(got[dead] == 0.0) and not np.signbit(got[dead]).any()
    return float((np.abs(got - want)[live] / mag[live]).max())


SEVEN = dict(axes=[3, 1, None, 2, 3, 1, 2], no_s=(2,), no_t=(4,), kinds=["ATAN", "TANH", "NONE", "SIGMOID", "NONE", "ATAN", "TANH"],
             clamps=[2.0, 1.5, 0.5, 2.0, 0.5, 2.0, 1.0])
CASES = [
    # odd sizes, an odd tail of the footprint loop, batch strides, pre_scale != 1 (D = 6 and 12)
    ((2, 3, 5, 7), dict(axes=[3, 1, None, 2, 3, 1], no_s=(2,), pres=[1.0, 0.1, 1.0, 0.7, 1.0, 1.3]), 1),
    ((2, 3, 5, 7), dict(axes=[3, 1, None, 2, 3, 1], no_s=(2,), pres=[1.0, 0.1, 1.0, 0.7, 1.0, 1.3]), 2),
    # seven stages, all clamp kinds, m = 1, 2, 3 (D = 8, 16, 32)
    ((2, 4, 8, 64), SEVEN, 1),
    ((2, 4, 8, 64), SEVEN, 2),
    ((2, 4, 8, 64), SEVEN, 3),
]


@pytest.mark.parametrize("shape,spec,m", CASES)
def test_kernel_vs_restatement(shape, spec, m):
    """The full box catalogue (one voxel, ragged range around whole blocks, whole depth, clipped, empty, both covariance signs, disjoint)
    and the diagonal, against the float64 restatement on the same fp32 inputs; a non-NULL t changes no bit."""
    B, C, H, W = shape
    ref = ref_chain(shape, seed=sum(shape) + m, **spec)
    boxes, pairs = M.box_catalogue(C << m, H, W)
    pr = all_pairs(boxes, pairs)
    got = run(dev_chain(ref), Z1, shape, m, boxes, pr)
    want, mag = M.step_term(ref, shape, m, Z1, boxes, pr)
    err = rel_to_terms(got, want, mag)
    print(f"[roi moments] kernel {shape} m={m}: error / sum of |terms| {err:.3e} (bound {VAR_BOUND:.3e}, ratio {err / VAR_BOUND:.3f})")
    assert err <= VAR_BOUND
    assert torch.equal(run(dev_chain(ref, with_t=False), Z1, shape, m, boxes, pr).nan_to_num(nan=-1.0), got.nan_to_num(nan=-1.0))
    R_ = len(boxes)
    if m == 2:                       # boxes 7, 8 are the two halves of a 4-block: negative at that level
        assert (got[:, R_ + 1] < 0).all()
    if m != 2:                       # boxes 5, 6 overlap: positive (at m = 2 box 6 is balanced over its block and the term is zero)
        assert (got[:, R_ + 0] > 0).all()


def test_exact_cases():
    from cwfa_amd import ops
    shape, m = (2, 4, 8, 64), 2
    B, C, H, W = shape
    ref = ref_chain(shape, seed=77, **SEVEN)
    dev = dev_chain(ref)
    boxes, pairs = M.box_catalogue(C << m, H, W)
    pr = all_pairs(boxes, pairs)
    R_ = len(boxes)
    got = run(dev, Z1, shape, m, boxes, pr)
    zero = torch.zeros(B, dtype=torch.float64, device="cuda")

    def bits(a, b):
        return torch.equal(a.view(torch.int64), b.view(torch.int64))

    assert bits(got[:, 2], zero)                             # the whole-depth box
    assert bits(got[:, R_ + 2], zero)                        # disjoint footprints
    assert bits(got[:, R_ + 5], zero)                        # a pair with the whole-depth box
    assert got[:, 4].isnan().all() and got[:, R_ + 4].isnan().all()      # the empty box and a pair with it
    assert (got[:, [0, 1, 3, 5, 7, 8, 9, 10]] > 0).all() and bits(got[:, 6], zero)      # [1, 3) is balanced over [0, 4)
    # z_var = 0: exactly zero, and the empty box is still NaN
    z0 = run(dev, 0.0, shape, m, boxes, pr)
    assert bits(z0.nan_to_num(nan=0.0), torch.zeros_like(z0)) and torch.equal(z0.isnan(), got.isnan())
    # two calls give the same bits; pairs = None is the explicit diagonal; the calls accumulate
    assert bits(run(dev, Z1, shape, m, boxes, pr), got)
    diag = run(dev, Z1, shape, m, boxes)
    assert bits(diag, got[:, :R_].contiguous())
    twice = run(dev, Z1, shape, m, boxes, out=diag.clone())
    assert torch.equal(twice.nan_to_num(nan=-1.0), (2 * diag).nan_to_num(nan=-1.0))
    # the device table and the kernel arguments carry the same boxes: same bits; 150 pairs take three launches of kernel arguments
    many = np.concatenate([pr] * 9)[:150]
    assert len(many) > 2 * ops.ROI_COV_ARG_PAIRS
    by_args = run(dev, Z1, shape, m, ops.RoiPairs(boxes, many, "cuda", device_table=False))
    by_table = run(dev, Z1, shape, m, ops.RoiPairs(boxes, many, "cuda", device_table=True))
    assert bits(by_args, by_table) and bits(by_args[:, :len(pr)].contiguous(), got) and bits(by_args[:, 136:150].contiguous(), got[:, :14].contiguous())
    # prepared tables serve every level
    rp = ops.RoiPairs(boxes, pr, "cuda", device_table=True)
    assert bits(run(dev, Z1, shape, m, rp), got)


def test_unread_channels_are_never_loaded():
    """Box 1 at D = 16 is the depth range [3, 9): the 4-block [4, 8) = channel 1 lies wholly inside, its q is 0 and the kernel skips it
    before any load.  Every s value that the walk from the counted (channel, y, x) positions does not reach -- all of channel 1's
    path among them -- is replaced by a huge finite value: no bit of the result changes."""
    shape, m = (2, 4, 8, 64), 2
    B, C, H, W = shape
    ref = ref_chain(shape, seed=78, **SEVEN)
    boxes, _ = M.box_catalogue(C << m, H, W)
    assert tuple(boxes[1][:2]) == (3, 9)
    pr = np.array([[1, 1], [1, 5], [5, 1]], dtype=np.int32)
    got = run(dev_chain(ref), Z1, shape, m, boxes, pr)
    mask = torch.zeros(C, H, W, dtype=torch.bool)
    for r1, r2 in pr:
        b1, b2 = boxes[r1], boxes[r2]
        qq = M.q_table(b1[0], b1[1], m, C) * M.q_table(b2[0], b2[1], m, C)
        for c in np.nonzero(qq)[0]:
            mask[c, max(b1[2], b2[2]):min(b1[3], b2[3]), max(b1[4], b2[4]):min(b1[5], b2[5])] = True
    assert mask[0].any() and mask[2].any() and not mask[1].any() and not mask[3].any()
    poisoned = [dict(st) for st in ref]
    n_poisoned = 0
    for st in reversed(poisoned):                             # the walk runs from the last stage back
        if st["s_raw"] is not None:
            s = st["s_raw"].clone()
            s[:, ~mask] = 3.0e38
            n_poisoned += int((~mask).sum())
            st["s_raw"] = s
        if st["perm"] is not None:                            # stage k reads at p, the stage before it at g_k(p)
            mask = torch.zeros_like(mask).index_copy_(st["axis"] - 1, st["perm"], mask)
    assert n_poisoned > 6 * (C * H * W - 64)
    again = run(dev_chain(poisoned), Z1, shape, m, boxes, pr)
    assert torch.equal(again.view(torch.int64), got.view(torch.int64)) and torch.isfinite(got).all() and (got[:, 0] > 0).all()


# ------------------------------------------------------------------------------------------------ the reference fixture
def _fixture_pyramid():
    """The package's own modules with the fixture's weights: (conv_inn, cond_nets, cond_input, mean_cache, low).  The condition nets
    are stand-ins that return the fixture's processed conditions; conv_inn[0] is the finest step."""
    from cwfa_amd import networks as N
    from test_host_logic import build_step
    fx = load_golden("g26_roi_moments")
    keep = N.networks_n_chans
    conv_inn, cond_nets, mean_cache = [], [], []
    try:
        for ix in (0, 1):
            _, g = build_step("CAT", ix, D=int(fx["D"]), H=int(fx["H"]), W=int(fx["W"]), n_ch=int(fx["n_ch"]), cond_ch=int(fx["cond_ch"]))
            g.load_state_dict(sd_of(fx, prefix=f"s{ix}/sd/"))
            for i, mod in enumerate(g.module_list):
                if f"s{ix}/meta/axis_{i}" in fx:
                    assert int(mod.axis) == int(fx[f"s{ix}/meta/axis_{i}"])
            conv_inn.append(g.eval().cuda())
            c0 = torch.from_numpy(fx[f"s{ix}/c0"]).cuda()
            cond_nets.append(lambda x, _c=c0: [_c])
            mean_cache.append(torch.from_numpy(fx[f"s{ix}/c1"]).cuda())
    finally:
        N.networks_n_chans = keep
    return fx, conv_inn, cond_nets, None, mean_cache, torch.from_numpy(fx["low"]).cuda()


def test_reference_fixture():
    """posterior_roi_moments through the package's modules against the reference's autograd: mean against the ROI means of the z = 0
    volume (4 * 2^-24 of the largest |mean| for the ROI sums of fp32 voxels, plus TOL = 1e-4, the bound the golden step tests hold the
    sub-networks' fp32 volume to); std^2 / z_var and cov / z_var against var_unit / cov_unit at FIX_BOUND of the sum of absolute terms."""
    from cwfa_amd import CWFA
    fx, conv_inn, cond_nets, cond_input, mean_cache, low = _fixture_pyramid()
    boxes, pairs = fx["boxes"], fx["pairs"]
    mean, std, cov, vol = CWFA.posterior_roi_moments(conv_inn, cond_nets, cond_input, mean_cache, boxes, low=low, temperature=1, pairs=pairs,
                                                     return_volume=True)
    assert mean.dtype == std.dtype == cov.dtype == torch.float64 and mean.shape == std.shape == (2, len(boxes)) and cov.shape == (2, len(pairs))
    assert torch.equal(vol, CWFA.posterior_moments(conv_inn, cond_nets, cond_input, mean_cache, low=low, temperature=1)[0])
    want_mean = fx["roi_mean0"]
    assert np.array_equal(np.isnan(want_mean), mean.isnan().cpu().numpy())
    e_mean = float(np.nanmax(np.abs(mean.cpu().numpy() - want_mean)) / np.nanmax(np.abs(want_mean)))
    e_var = rel_to_terms(std ** 2 / Z1, fx["var_unit"], np.nan_to_num(fx["abs_unit_var"], nan=1.0))
    e_cov = rel_to_terms(cov / Z1, fx["cov_unit"], np.nan_to_num(fx["abs_unit_cov"], nan=1.0))
    print(f"[roi moments] fixture: mean {e_mean:.3e} (bound {TOL + 4 * 2.0 ** -24:.3e}), var {e_var:.3e}, cov {e_cov:.3e} (bound {FIX_BOUND:.3e}, "
          f"ratios {e_var / FIX_BOUND:.3f}, {e_cov / FIX_BOUND:.3f})")
    assert e_mean <= TOL + 4 * 2.0 ** -24
    assert e_var <= FIX_BOUND and e_cov <= FIX_BOUND
    assert (cov[:, 0] > 0).all() and (cov[:, 1] < 0).all() and not cov[:, 2].any() and not std[:, 2].any()
    # without pairs there is no cov; the moments are the same bits
    m2, s2, c2 = CWFA.posterior_roi_moments(conv_inn, cond_nets, cond_input, mean_cache, boxes, low=low, temperature=1)
    assert c2 is None and torch.equal(m2.nan_to_num(nan=-1.0), mean.nan_to_num(nan=-1.0)) and torch.equal(s2.nan_to_num(nan=-1.0), std.nan_to_num(nan=-1.0))
    # std_scale: one power on mean and std, two on cov
    k = 2.5
    mk, sk, ck = CWFA.posterior_roi_moments(conv_inn, cond_nets, cond_input, mean_cache, boxes, low=low, temperature=1, pairs=pairs, std_scale=k)
    live, livec = ~mean.isnan(), ~cov.isnan()
    for a, b, scale in ((mk[live], mean[live], k), (sk[live], std[live], k), (ck[livec], cov[livec], k * k)):
        assert float(((a - scale * b).abs() / (scale * b).abs().clamp_min(1e-300)).max()) <= 1e-15
    # temperature 0: no spread, the same mean
    m0, s0, c0 = CWFA.posterior_roi_moments(conv_inn, cond_nets, cond_input, mean_cache, boxes, low=low, temperature=0, pairs=pairs)
    assert not s0[live].any() and not c0[livec].any() and s0[~live].isnan().all() and torch.equal(m0[live], mean[live])
    with pytest.raises(ValueError):
        CWFA.posterior_roi_moments(conv_inn, cond_nets, cond_input, mean_cache, boxes, low=low, std_scale=0.0)


def test_one_voxel_boxes_vs_per_voxel_route():
    """std^2 of one-voxel boxes from posterior_roi_moments and posterior_moments(keep_all=False)^2 at those voxels, on the two-step
    pyramid of the g26 modules.  Both are held to the float64 value from the CPU oracle's coefficients (one voxel: the sum of the
    absolute terms IS the value): the ROI route at FIX_BOUND; the per-voxel route at FIX_BOUND + 2^-22, because it returns the fp32
    square root of its variance and squaring doubles that rounding.  Hence they differ by no more than the sum of the two."""
    from cwfa_amd import CWFA
    from test_roi_moments_cpu import fixture_steps
    fx, conv_inn, cond_nets, cond_input, mean_cache, low = _fixture_pyramid()
    D, H, W = int(fx["D"]), int(fx["H"]), int(fx["W"])
    rs = np.random.RandomState(5)
    vox = np.stack([rs.randint(0, D, 40), rs.randint(0, H, 40), rs.randint(0, W, 40)], 1)
    vox[:4] = [[0, 0, 0], [D - 1, H - 1, W - 1], [3, 0, W - 1], [4, H - 1, 0]]
    boxes = np.stack([vox[:, 0], vox[:, 0] + 1, vox[:, 1], vox[:, 1] + 1, vox[:, 2], vox[:, 2] + 1], 1).astype(np.int32)
    T = 0.8
    zv = CWFA.truncated_normal_variance(T)
    mean, std, _ = CWFA.posterior_roi_moments(conv_inn, cond_nets, cond_input, mean_cache, boxes, low=low, temperature=T)
    vmean, vstd = CWFA.posterior_moments(conv_inn, cond_nets, cond_input, mean_cache, low=low, temperature=T)
    idx = (slice(None), torch.from_numpy(vox[:, 0]), torch.from_numpy(vox[:, 1]), torch.from_numpy(vox[:, 2]))
    assert torch.equal(mean, vmean.cpu()[idx].double().cuda())                  # the mean of one voxel is that voxel
    want, _ = M.roi_cov(fixture_steps(fx), zv, boxes)
    want = torch.from_numpy(want)
    roi_var, vox_var = (std ** 2).cpu(), vstd.cpu()[idx].double() ** 2
    e_roi, e_vox = float(((roi_var - want).abs() / want).max()), float(((vox_var - want).abs() / want).max())
    e_both = float(((roi_var - vox_var).abs() / want).max())
    print(f"[roi moments] one voxel: ROI route {e_roi:.3e}, per-voxel route {e_vox:.3e}, between them {e_both:.3e} (bound {FIX_BOUND:.3e})")
    assert e_roi <= FIX_BOUND and e_vox <= FIX_BOUND + 2.0 ** -22 and e_both <= 2 * FIX_BOUND + 2.0 ** -22


def test_other_block_types_raise():
    from cwfa_amd import CWFA
    conv_inn, cond_nets, cond_input, mean_cache, low = _pyramid("GLOW")
    with pytest.raises(NotImplementedError, match="affine"):
        CWFA.posterior_roi_moments(conv_inn, cond_nets, cond_input, mean_cache, [[0, 1, 0, 1, 0, 1]], low=low)


# ------------------------------------------------------------------------------------------------ the seeded sampler
def test_samples_agree_with_closed_form():
    """Two hand-built steps, C0 = 2, H = 8, W = 64 (D = 8), T = 1, N = 2048 seeded samples through ops.chain_inv_samples and
    ops.roi_means.  24 boxes with pairwise disjoint 4 x 4 footprints (none whole-depth: every variance is positive) share no latent,
    so their ratios r_i = sample variance / closed form are independent; an ROI mean is a sum of scaled truncated normals, whose
    kurtosis is below a normal's, so sd(r_i) <= sqrt(2 / (N - 1)).  Required: |mean_i r_i - 1| <= 6 sqrt(2 / ((N - 1) 24)) = 0.038, each
    |r_i - 1| <= 6 sqrt(2 / (N - 1)) = 0.19, each sample mean within 6 std / sqrt N of the closed-form mean, the sample covariance of
    one overlapping pair of each sign within 6 sqrt((s1^2 s2^2 + cov^2) / (N - 1)) (the normal-theory sd of a sample covariance), and
    a 25th, whole-depth box has a sample variance below 1e-10 of the others' mean (fp32 rounding of the volume only)."""
    from cwfa_amd import CWFA, ops
    sa, sb = (1, 2, 8, 64), (1, 4, 8, 64)
    N, T, seed = 2048, 1.0, 31
    axes = [None, 3, 1, 2, 3, 1]
    dev_a, dev_b = dev_chain(ref_chain(sa, axes, 91)), dev_chain(ref_chain(sb, axes, 92))
    low = torch.randn(sa, generator=torch.Generator().manual_seed(93)).cuda()
    ranges = [(1, 7), (3, 4), (2, 5), (0, 6), (5, 8), (2, 3)]
    feet = [(y, y + 4, x, x + 4) for y in (0, 4) for x in range(0, 64, 4)]
    boxes = [[*ranges[i % 6], *feet[i]] for i in range(24)] + [[0, 8, *feet[24]]]
    boxes += [[0, 3, 0, 4, 40, 44], [0, 3, 1, 5, 41, 45], [0, 2, 4, 8, 48, 52], [2, 4, 4, 8, 48, 52]]        # 25, 26: +   27, 28: -
    boxes = np.array(boxes, dtype=np.int32)
    pairs = np.array([[25, 26], [27, 28]], dtype=np.int32)
    traces = []
    for k in range(0, N, 256):
        xa = ops.chain_inv_samples(low, dev_a, 256, T, seed, stream=0, sample_offset=k)
        xb = ops.chain_inv_samples(xa, dev_b, 256, T, seed, stream=1, sample_offset=k)
        traces.append(ops.roi_means(xb.view(256, 8, 8, 64), boxes))
    traces = torch.cat(traces, 1).cpu().numpy()              # [R, N]
    zv = CWFA.truncated_normal_variance(T)
    var = torch.zeros(1, len(boxes), dtype=torch.float64, device="cuda")
    ops.chain_inv_roi_cov(var, dev_a, zv, sa, 2, boxes)
    ops.chain_inv_roi_cov(var, dev_b, zv, sb, 1, boxes)
    cov = torch.zeros(1, 2, dtype=torch.float64, device="cuda")          # the pairs: a separate call
    ops.chain_inv_roi_cov(cov, dev_a, zv, sa, 2, boxes, pairs)
    ops.chain_inv_roi_cov(cov, dev_b, zv, sb, 1, boxes, pairs)
    var, cov = var.cpu().numpy()[0], cov.cpu().numpy()[0]
    mean = ops.roi_means(ops.chain_inv(None, ops.chain_inv(None, low, dev_a), dev_b)[0:1].view(1, 8, 8, 64), boxes).cpu().numpy()[:, 0]
    svar = traces.var(axis=1, ddof=1)
    r = svar[:24] / var[:24]
    print(f"[roi moments] samples: mean ratio {r.mean():.4f} (|.-1| <= {6 * math.sqrt(2 / ((N - 1) * 24)):.4f}), worst box {np.abs(r - 1).max():.4f} "
          f"(<= {6 * math.sqrt(2 / (N - 1)):.4f}), whole-depth {svar[24] / svar[:24].mean():.2e}")
    assert (var[:24] > 0).all() and var[24] == 0.0
    assert abs(r.mean() - 1.0) <= 6 * math.sqrt(2.0 / ((N - 1) * 24))
    assert np.abs(r - 1.0).max() <= 6 * math.sqrt(2.0 / (N - 1))
    assert svar[24] <= 1e-10 * svar[:24].mean()
    assert (np.abs(traces.mean(axis=1) - mean) <= 6 * np.sqrt(var / N) + 1e-5).all()       # (+ fp32 rounding of the volume)
    assert cov[0] > 0 and cov[1] < 0
    for p, (r1, r2) in enumerate(pairs):
        scov = float(np.cov(traces[r1], traces[r2], ddof=1)[0, 1])
        sd = math.sqrt((var[r1] * var[r2] + cov[p] ** 2) / (N - 1))
        print(f"[roi moments] pair {p}: sample covariance {scov:.5e}, closed form {cov[p]:.5e}, 6 sd {6 * sd:.3e}")
        assert abs(scov - cov[p]) <= 6 * sd


# ------------------------------------------------------------------------------------------------ validation
def test_errors():
    """Every rejected call returns the ABI's error before a launch: `out` keeps its zeros."""
    from cwfa_amd import ops
    from cwfa_amd._lib import CwfaHipError
    shape, m = (1, 3, 5, 7), 1
    ref = ref_chain(shape, [3, 1, None], 5)
    dev = dev_chain(ref)
    out = torch.zeros(1, 1, dtype=torch.float64, device="cuda")
    ok = [[0, 3, 0, 5, 0, 7]]
    for bad in ([[0, 7, 0, 5, 0, 7]], [[0, 3, 0, 6, 0, 7]], [[0, 3, 0, 5, -1, 7]], [[3, 2, 0, 5, 0, 7]]):
        with pytest.raises(CwfaHipError, match="not inside"):
            ops.chain_inv_roi_cov(out, dev, Z1, shape, m, bad)
    with pytest.raises(CwfaHipError, match="outside"):
        ops.chain_inv_roi_cov(out, dev, Z1, shape, m, ok, [[0, 1]])
    with pytest.raises(ValueError, match="outside"):
        ops.RoiPairs(ok, [[0, 1]], "cuda", device_table=True)
    with pytest.raises(CwfaHipError, match="level"):
        ops.chain_inv_roi_cov(out, dev, Z1, shape, 0, ok)
    gin = dev[:2] + [ops.stage(ref[2]["s_raw"].cuda(), None, gin=True)]
    with pytest.raises(CwfaHipError, match="GIN"):
        ops.chain_inv_roi_cov(out, gin, Z1, shape, m, ok)
    for zv in (-0.1, float("nan"), float("inf")):
        with pytest.raises(CwfaHipError, match="z_var"):
            ops.chain_inv_roi_cov(out, dev, zv, shape, m, ok)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.chain_inv_roi_cov(torch.zeros(1, 1, dtype=torch.float64), dev, Z1, shape, m, ok)
    with pytest.raises(TypeError):
        ops.chain_inv_roi_cov(torch.zeros(1, 1, device="cuda"), dev, Z1, shape, m, ok)
    with pytest.raises(ValueError):
        ops.chain_inv_roi_cov(torch.zeros(1, 2, dtype=torch.float64, device="cuda"), dev, Z1, shape, m, ok)
    assert not out.any()
    # empty problems launch nothing; a chain without stages is v = z: z_var / (2 cnt) for one depth of a pair
    assert ops.chain_inv_roi_cov(torch.zeros(1, 0, dtype=torch.float64, device="cuda"), dev, Z1, shape, m, np.zeros((0, 6), dtype=np.int32)).numel() == 0
    plain = ops.chain_inv_roi_cov(out, [], Z1, shape, m, [[0, 1, 0, 5, 0, 7]])
    assert abs(float(plain) - float(np.float32(Z1)) / (2 * 35)) <= 1e-17                  # (z_var crosses the ABI as a float)
