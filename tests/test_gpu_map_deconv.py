"""GPU: MAP Richardson-Lucy, XLFMDeconv under a per-voxel Gaussian prior.

The two new update kernels of csrc/deconv_ops.hip alone against a numpy fp32 emulation of the M-step, operation by operation
(np.sqrt and / on float32 are IEEE, as the pinned device forms are): bits equal; the penalty against its float64 sum within
n 2^-53 sum|terms|, the bound of any order of n float64 additions of identical terms; the finish kernel on top of what the trace
held.  Then XLFMDeconv with a prior on the fixtures recorded from the reference (tests/golden/g25_deconv_rl_*.npz) against the
float64 restatement tests/map_deconv_ref.py: max|gpu - f64| <= 8 dev_ref max|f64|, dev_ref the fp32 CPU restatement's own distance
from the float64 one on the same inputs (computed here, itself <= 2e-5), 8 the margin of tests/test_gpu_deconv.py."""
import functools

import numpy as np
import pytest
import torch

import accel_deconv_ref as A
import deconv_ref as R
import map_deconv_ref as M
from test_deconv_cpu import RL, rel, rl
from test_gpu_deconv import bits, deconv_args, dev, host

pytestmark = pytest.mark.gpu
MARGIN = 8.0
N_IT = 8
f32 = np.float32
# (F, obj, D, depths per launch): element by element with the slabs accumulated over chunks of 2 + 1 depths; 16-byte groups; two
# blocks per depth in the accelerated walk (72 * 18 = 1296 groups of 1024 per block) and six in the plain one, the last ragged
SHAPES = [(9, 5, 3, 2), (16, 8, 3, 3), (96, 72, 2, 2)]


def np_m_step(a, mu, w):
    """The M-step in numpy float32, one rounding per operation, in the kernel's order."""
    with np.errstate(all="ignore"):
        c = f32(1) - w * mu
        t = c * c + f32(4) * (w * a)
        r = np.sqrt(np.where(t < 0, f32(0), t))
        out = np.where(c > 0, (f32(2) * a) / (c + r), (r - c) / (f32(2) * w))
    assert out.dtype == np.float32
    return out


def np_penalty_terms(y, mu, w):
    d = y.astype(np.float64) - mu.astype(np.float64)
    return 0.5 * w.astype(np.float64) * (d * d)


def kernel_inputs(F, obj, D):
    rng = np.random.default_rng(F + obj)
    po = (F - obj) // 2
    win = (slice(None), slice(None), slice(po, po + obj), slice(po, po + obj))
    shape = (1, D, obj, obj)
    y_h = np.zeros((1, D, F, F), dtype=f32)
    y_h[win] = np.abs(rng.standard_normal(shape)).astype(f32)
    b_h = (1 + 0.3 * rng.standard_normal((1, D, F, F))).astype(f32)
    idx = R.np_shift_index(F)
    inside = np.zeros((F, F), dtype=bool)
    inside[np.ix_(idx[po:po + obj], idx[po:po + obj])] = True
    b_h[:, :, ~inside] = np.nan                                                          # whatever lies outside the window is not used
    # w over two decades, w mu over a factor 5 to either side of 1 (the branch), one mean in eight negative, one w in ten zero
    w_h = (10.0 ** rng.uniform(-1, 1, shape)).astype(f32)
    mu_h = ((10.0 ** rng.uniform(-0.7, 0.7, shape)) / w_h).astype(f32)
    mu_h[rng.random(shape) < 0.125] *= f32(-1)
    w_h[rng.random(shape) < 0.1] = 0
    # planted: a voxel at 0 stays 0 where c > 0, is revived at mu - 1 / w where c < 0, and c == 0 is 0, not 0 / 0
    y_h[0, 0, po, po:po + 3] = 0
    w_h[0, 0, 0, :3], mu_h[0, 0, 0, :3] = (1, 1, 0.5), (0.5, 4, 2)
    y_h[0, D - 1, po + obj - 1, po + obj - 1] = 0
    # and a back projection below zero under a prior: c * c + 4 w a = 0.01 - 2 < 0 is held at 0, the result 2a / c, not NaN
    y_h[0, D - 1, po + 1, po + 1], b_h[0, D - 1, idx[po + 1], idx[po + 1]] = 1, -0.5
    w_h[0, D - 1, 1, 1], mu_h[0, D - 1, 1, 1] = 1, 0.9
    m_h = b_h[:, :, idx][:, :, :, idx][win]
    return po, win, y_h, b_h, m_h, mu_h, w_h


def check_shares(y_win, m_h, mu_h, w_h, out):
    c = f32(1) - w_h * mu_h
    n = c.size
    first, second, zero_w = (c > 0).sum() / n, (c <= 0).sum() / n, (w_h == 0).sum() / n
    assert first >= 0.25 and second >= 0.25 and zero_w >= 0.05, (first, second, zero_w)
    assert c[0, 0, 0, 0] > 0 and c[0, 0, 0, 1] < 0 and c[0, 0, 0, 2] == 0 and not y_win[0, 0, 0, :3].any()
    assert out[0, 0, 0, :3].tolist() == [0.0, 3.0, 0.0], "stays 0, revived at mu - 1 / w, 0 and not 0 / 0"
    assert not np.isnan(out).any(), "no NaN where the inputs have none"
    assert y_win[0, -1, 1, 1] * m_h[0, -1, 1, 1] == f32(-0.5) and abs(out[0, -1, 1, 1] + 10) < 1e-5, "a back projection below zero"


def border_is_zero(got, F, obj, po):
    border = np.ones((F, F), dtype=bool)
    border[po:po + obj, po:po + obj] = False
    return (bits(got[:, :, border]) == 0).all()


def check_penalty(ops, slab, terms, chunk, D, blocks_per_depth):
    n = terms.size
    s_h = host(slab)
    err, bound = abs(s_h.sum() - terms.sum()), n * 2.0 ** -53 * np.abs(terms).sum()
    print(f"penalty {terms.sum():.6f} off by {err:.3e} (bound {bound:.3e})")
    assert err <= bound and terms.sum() > 0
    used = np.flatnonzero(s_h)
    assert used.size and used.max() < chunk * blocks_per_depth, "one row per (depth of a chunk, block): the second chunk added to the first's"
    trace = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    trace[2] = 123.456
    ops.deconv_penalty(slab, trace, 2)
    t_h = host(trace)
    assert abs(t_h[2] - (123.456 + terms.sum())) <= bound + 2.0 ** -52 * abs(t_h[2]), "added onto what the trace held"
    assert (t_h[[0, 1, 3]] == -7.0).all() and not slab.any(), "one element is touched and the slab is zeroed"
    return t_h[2]


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("F,obj,D,chunk", SHAPES)
def test_update_map(F, obj, D, chunk):
    from cwfa_amd import ops
    po, win, y_h, b_h, m_h, mu_h, w_h = kernel_inputs(F, obj, D)
    want = np_m_step(y_h[win] * m_h, mu_h, w_h)
    check_shares(y_h[win], m_h, mu_h, w_h, want)
    y, b, mu, w = dev(y_h), dev(b_h), dev(mu_h), dev(w_h)
    slab = ops.deconv_penalty_slab(chunk, obj, "cuda")
    assert slab.shape == (chunk * -(-obj * obj // 256),) and slab.dtype == torch.float64 and not slab.any()
    for jj in range(0, D, chunk):
        ops.deconv_update_map(y[:, jj:jj + chunk], b[:, jj:jj + chunk], mu[:, jj:jj + chunk], w[:, jj:jj + chunk], obj, po, slab)
    got = host(y)
    assert np.array_equal(bits(got[win]), bits(want)), "nine fp32 operations, each rounded once"
    assert border_is_zero(got, F, obj, po), "the border stays exactly +0.0"
    assert np.array_equal(bits(host(b)), bits(b_h)) and np.array_equal(bits(host(mu)), bits(mu_h)) and np.array_equal(bits(host(w)), bits(w_h))
    plain = host(ops.deconv_update(dev(y_h), dev(np.nan_to_num(b_h)), obj, po))[win]
    assert (w_h == 0).sum() >= 3 and np.array_equal(bits(got[win][w_h == 0]), bits(plain[w_h == 0])), "w = 0 is deconv_update"
    vec = F % 4 == 0 and obj % 4 == 0 and po % 4 == 0 and ((F + 1) // 2) % 4 == 0
    first = check_penalty(ops, slab, np_penalty_terms(y_h[win], mu_h, w_h), chunk, D, -(-(obj * obj // 4 if vec else obj * obj) // 256))
    # without a slab: the same bits, no reduction; and the penalty is bitwise repeatable
    y2 = dev(y_h)
    for jj in range(0, D, chunk):
        ops.deconv_update_map(y2[:, jj:jj + chunk], b[:, jj:jj + chunk], mu[:, jj:jj + chunk], w[:, jj:jj + chunk], obj, po)
    assert np.array_equal(bits(host(y2)), bits(got)) and not slab.any()
    # NaN is kept, not turned into 0 by the discriminant's maximum: in the back projection on either branch, in mu, in w
    idx = R.np_shift_index(F)
    b_n, mu_n, w_n = b_h.copy(), mu_h.copy(), w_h.copy()
    b_n[0, D - 1, idx[po + 2], idx[po + 2]] = b_n[0, D - 1, idx[po + 2], idx[po + 3]] = np.nan
    w_n[0, D - 1, 2, 2:4], mu_n[0, D - 1, 2, 2:4] = 1, (0.5, 4)
    mu_n[0, D - 1, 3, 2], w_n[0, D - 1, 3, 3] = np.nan, np.nan
    planted = np.zeros(want.shape, dtype=bool)
    planted[0, D - 1, 2, 2:4] = planted[0, D - 1, 3, 2:4] = True
    want_n = np_m_step(y_h[win] * b_n[:, :, idx][:, :, :, idx][win], mu_n, w_n)
    got_n = host(ops.deconv_update_map(dev(y_h), dev(b_n), dev(mu_n), dev(w_n), obj, po))
    assert np.array_equal(np.isnan(got_n[win]), planted) and np.array_equal(np.isnan(want_n), planted), "NaN exactly where one went in"
    assert np.array_equal(bits(got_n[win][~planted]), bits(want[~planted])) and border_is_zero(got_n, F, obj, po)
    y3 = dev(y_h)
    for jj in range(0, D, chunk):
        ops.deconv_update_map(y3[:, jj:jj + chunk], b[:, jj:jj + chunk], mu[:, jj:jj + chunk], w[:, jj:jj + chunk], obj, po, slab)
    trace = torch.tensor([0.0, 0.0, 123.456, 0.0], dtype=torch.float64, device="cuda")
    ops.deconv_penalty(slab, trace, 2)
    assert host(trace)[2] == first


@pytest.mark.parametrize("F,obj,D,chunk", SHAPES)
def test_update_accel_map(F, obj, D, chunk):
    from cwfa_amd import ops
    po, win, y_h, b_h, m_h, mu_h, w_h = kernel_inputs(F, obj, D)
    xn_want = np_m_step(y_h[win] * m_h, mu_h, w_h)
    check_shares(y_h[win], m_h, mu_h, w_h, xn_want)
    g_want = xn_want - y_h[win]
    rng = np.random.default_rng(F)
    gp_h = (f32(2) * g_want + 0.1 * rng.standard_normal(g_want.shape).astype(f32)).astype(f32)
    y, b, mu, w, g = dev(y_h), dev(b_h), dev(mu_h), dev(w_h), dev(gp_h)
    xn = torch.full((1, D, obj, obj), np.nan, device="cuda")
    slab, pen = ops.deconv_accel_slab(chunk, obj, "cuda"), ops.deconv_penalty_slab(chunk, obj, "cuda")
    for jj in range(0, D, chunk):
        s = slice(jj, jj + chunk)
        ops.deconv_update_accel_map(y[:, s], b[:, s], g[:, s], xn[:, s], mu[:, s], w[:, s], slab, obj, po, pen)
    assert np.array_equal(bits(host(xn)), bits(xn_want)), "the M-step of the single fp32 product"
    assert np.array_equal(bits(host(g)), bits(g_want)), "one fp32 difference, written over the previous step"
    assert np.array_equal(bits(host(y)), bits(y_h)) and np.array_equal(bits(host(b)), bits(b_h)), "inputs are only read"
    assert np.array_equal(bits(host(mu)), bits(mu_h)) and np.array_equal(bits(host(w)), bits(w_h))
    plain = host(ops.deconv_update(dev(y_h), dev(np.nan_to_num(b_h)), obj, po))[win]
    assert np.array_equal(bits(host(xn)[w_h == 0]), bits(plain[w_h == 0])), "w = 0 is deconv_update"
    same = ops.deconv_update_map(dev(y_h), b, mu, w, obj, po)
    assert np.array_equal(bits(host(same)[win]), bits(host(xn))), "and the plain form's bits everywhere"

    n = D * obj * obj
    t_num, t_den = g_want.astype(np.float64) * gp_h.astype(np.float64), gp_h.astype(np.float64) ** 2
    s_h = host(slab)
    e_num, e_den = abs(s_h[:, 0].sum() - t_num.sum()), abs(s_h[:, 1].sum() - t_den.sum())
    b_num, b_den = n * 2.0 ** -53 * np.abs(t_num).sum(), n * 2.0 ** -53 * t_den.sum()
    print(f"F={F} obj={obj}: sum g g_prev off by {e_num:.3e} (bound {b_num:.3e}), sum g_prev^2 by {e_den:.3e} (bound {b_den:.3e})")
    assert e_num <= b_num and e_den <= b_den
    alpha = torch.full((1,), np.nan, device="cuda")
    ops.deconv_alpha(slab, 0.999, alpha)                                                 # alpha_kernel as it is, on the same columns
    q = t_num.sum() / t_den.sum()
    assert abs(float(host(alpha)[0]) - q) <= q * (2.0 ** -24 + b_num / abs(t_num.sum()) + b_den / t_den.sum() + 2.0 ** -52) and not slab.any()
    vec = F % 4 == 0 and obj % 4 == 0 and po % 4 == 0 and ((F + 1) // 2) % 4 == 0
    check_penalty(ops, pen, np_penalty_terms(y_h[win], mu_h, w_h), chunk, D, -(-(obj * obj // 4 if vec else obj * obj) // 1024))
    # without a penalty slab: the same bits
    g2, xn2 = dev(gp_h), torch.full((1, D, obj, obj), np.nan, device="cuda")
    for jj in range(0, D, chunk):
        s = slice(jj, jj + chunk)
        ops.deconv_update_accel_map(y[:, s], b[:, s], g2[:, s], xn2[:, s], mu[:, s], w[:, s], slab, obj, po)
    assert np.array_equal(bits(host(xn2)), bits(xn_want)) and np.array_equal(bits(host(g2)), bits(g_want)) and not pen.any()


def test_wrappers_refuse_wrong_tensors():
    from cwfa_amd import ops
    o, v = torch.zeros(1, 2, 16, 16, device="cuda"), torch.zeros(1, 2, 8, 8, device="cuda")
    slab, pen, tr = ops.deconv_accel_slab(2, 8, "cuda"), ops.deconv_penalty_slab(2, 8, "cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="mu .* does not hold 2 windows of 8 x 8"):
        ops.deconv_update_map(o, o.clone(), v[:, :1], v.clone(), 8, 4)
    with pytest.raises(ValueError, match="w .* does not hold"):
        ops.deconv_update_map(o, o.clone(), v, v[:, :, :4].contiguous(), 8, 4)
    with pytest.raises(ValueError, match="one shape"):
        ops.deconv_update_map(o, o[:, :1].clone(), v, v.clone(), 8, 4)
    with pytest.raises(TypeError, match="float32"):
        ops.deconv_update_map(o, o.clone(), v.double(), v.clone(), 8, 4)
    with pytest.raises(ValueError, match="contiguous"):
        ops.deconv_update_map(o, o.clone(), v, v.clone().transpose(2, 3), 8, 4)
    with pytest.raises(ValueError, match="penalty_slab"):
        ops.deconv_update_map(o, o.clone(), v, v.clone(), 8, 4, pen.float())
    with pytest.raises(RuntimeError, match="penalty slab holds 1 rows"):
        ops.deconv_update_map(o, o.clone(), v, v.clone(), 8, 4, pen[:1])
    with pytest.raises(RuntimeError, match="shares no buffer"):
        ops.deconv_update_map(v, v.clone(), v, v.clone(), 8, 0)
    with pytest.raises(ValueError, match="mu .* does not hold"):
        ops.deconv_update_accel_map(o, o.clone(), v, v.clone(), v[:, :1], v.clone(), slab, 8, 4)
    with pytest.raises(ValueError, match="slab"):
        ops.deconv_update_accel_map(o, o.clone(), v, v.clone(), v.clone(), v.clone(), slab.float(), 8, 4)
    with pytest.raises(RuntimeError, match="share no buffer"):
        ops.deconv_update_accel_map(o, o.clone(), v, v.clone(), v.clone(), v, slab, 8, 4)
    with pytest.raises(RuntimeError, match="penalty slab holds 1 rows"):
        ops.deconv_update_accel_map(o, o.clone(), v, v.clone(), v.clone(), v.clone(), slab, 8, 4, pen[:1])
    with pytest.raises(ValueError, match="trace"):
        ops.deconv_penalty(pen, tr.float(), 0)
    with pytest.raises(ValueError, match="not inside a trace"):
        ops.deconv_penalty(pen, tr, 3)
    with pytest.raises(ValueError, match="penalty_slab"):
        ops.deconv_penalty(slab.float(), tr, 0)


def test_map_offsets_beyond_2_31_elements():
    """One launch of each new update kernel over 130 planes of 4096 x 4096 (2^31 + 2^25 floats), zero except in the last plane, where
    a 32-bit offset would wrap to the front."""
    from cwfa_amd import ops
    D, S, obj, po = 130, 4096, 2048, 1024
    last = torch.randn(S, S, device="cuda")
    m_last = R.shift(last[None, None])[0, 0, po:po + obj, po:po + obj]
    obj_pad, b = torch.zeros(1, D, S, S, device="cuda"), torch.zeros(1, D, S, S, device="cuda")
    obj_pad[0, D - 1, po:po + obj, po:po + obj] = 2.0
    b[0, D - 1] = last
    mu, w, g, xn = (torch.zeros(1, D, obj, obj, device="cuda") for _ in range(4))
    mu[0, D - 1] = 3.0 * torch.rand(obj, obj, device="cuda")
    w[0, D - 1] = 0.5
    g[0, D - 1] = torch.randn(obj, obj, device="cuda")
    gp = g[0, D - 1].clone()
    x_want = torch.from_numpy(np_m_step(host(2.0 * m_last), host(mu[0, D - 1]), host(w[0, D - 1])))   # numpy's IEEE square root, division
    assert (1 - 0.5 * mu[0, D - 1] > 0).any() and (1 - 0.5 * mu[0, D - 1] <= 0).any() and not torch.isnan(x_want).any()
    p_want = (0.25 * (2.0 - mu[0, D - 1].double()) ** 2).sum().item()
    slab, pen = ops.deconv_accel_slab(D, obj, "cuda"), ops.deconv_penalty_slab(D, obj, "cuda")
    trace = torch.zeros(2, dtype=torch.float64, device="cuda")

    ops.deconv_update_accel_map(obj_pad, b, g, xn, mu, w, slab, obj, po, pen)
    assert torch.equal(xn[0, D - 1].cpu(), x_want) and torch.equal(g[0, D - 1].cpu(), x_want - 2.0)
    assert not xn[0, :D - 1].any() and not g[0, :D - 1].any(), "nothing wrapped to the front"
    num, den = (g[0, D - 1].double() * gp.double()).sum().item(), (gp.double() ** 2).sum().item()
    got = slab.sum(0).tolist()
    assert abs(got[0] - num) <= 1e-9 * abs(den) and abs(got[1] - den) <= 1e-9 * den
    ops.deconv_penalty(pen, trace, 0)
    assert abs(trace[0].item() - p_want) <= 1e-9 * p_want and not pen.any()

    ops.deconv_update_map(obj_pad, b, mu, w, obj, po, pen)
    assert torch.equal(obj_pad[0, D - 1, po:po + obj, po:po + obj].cpu(), x_want)
    assert not obj_pad[0, :D - 1].any(), "nothing wrapped to the front"
    ops.deconv_penalty(pen, trace, 1)
    assert abs(trace[1].item() - p_want) <= 1e-9 * p_want
    obj_pad[0, D - 1, po:po + obj, po:po + obj] = 0
    assert not obj_pad[0, D - 1].any(), "the border of the last plane stays 0"


# ------------------------------------------------------------------------------------------------ XLFMDeconv on the fixtures
def fixture_args(name, ns):
    z = rl(name)
    return (torch.from_numpy(z["OTF"]), torch.from_numpy(z["img"]), N_IT, [int(v) for v in z["ObjSize"]], [int(v) for v in z["ROIsize"]], ns,
            int(z["mult"]))


@functools.lru_cache(maxsize=None)
def prior_of(name, ns):
    """(mu, sigma, start) of the recipe, from the plain loop's float64 result: computed once, shared, never written."""
    plain = A.xlfm_deconv_accel(*fixture_args(name, ns), torch.float64, accelerate=False)[0]
    return M.prior_recipe(plain.numpy())


@functools.lru_cache(maxsize=None)
def restated(name, ns, accelerate, start):
    """The float64 restatement with the prior and the fp32 CPU restatement's distance from it: computed once, shared."""
    mu, sd, init = (torch.from_numpy(v.copy()) for v in prior_of(name, ns))
    kw = dict(accelerate=accelerate, prior_mean=mu, prior_std=sd, init=init if start else None)
    r64 = M.xlfm_deconv_map(*fixture_args(name, ns), torch.float64, **kw)
    r32 = M.xlfm_deconv_map(*fixture_args(name, ns), torch.float32, **kw)
    assert r64[4] == r32[4] == N_IT
    return r64, rel(r32[0].numpy(), r64[0].numpy()), rel(r32[1].numpy(), r64[1].numpy())


CASES = [(n, s) for n in RL for s in RL[n]]


@pytest.mark.parametrize("start", [False, True], ids=["ones", "init"])
@pytest.mark.parametrize("accelerate", [False, True], ids=["plain", "accel"])
@pytest.mark.parametrize("name,ns", CASES)
def test_map_deconv_matches_the_float64_restatement(name, ns, accelerate, start):
    from cwfa_amd import utils as U
    z = rl(name)
    r64, dev_vol, dev_est = restated(name, ns, accelerate, start)
    assert dev_vol <= 2e-5 and dev_est <= 2e-5, "the yardstick's own fp32 distance"
    mu_h, sd_h, init_h = prior_of(name, ns)
    branch = ((f32(1) / (sd_h * sd_h)) * mu_h >= 1).mean()
    assert 0.25 <= branch <= 0.45 and 0.05 <= np.isinf(sd_h).mean() <= 0.15, "both branches and voxels without a prior"
    OTF, img, mu, sd = dev(z["OTF"]), dev(z["img"]), dev(mu_h), dev(sd_h)
    init = dev(init_h) if start else None
    kw = dict(n_split_fourier=ns, accelerate=accelerate, trace=True, prior_mean=mu, prior_std=sd, init=init, **deconv_args(z))
    out = U.XLFMDeconv(OTF, img, N_IT, **kw)
    again = U.XLFMDeconv(OTF, img, N_IT, **kw)
    assert len(out) == 6 and out[1] == 0 and out[4] == r64[2] and out[5] == r64[3]
    vol, est = host(out[0]), host(out[2])
    assert vol.shape == tuple(r64[0].shape) and est.shape == tuple(r64[1].shape)
    e_vol, e_est = rel(vol, r64[0].numpy()), rel(est, r64[1].numpy())
    print(f"{name} n_split_fourier={ns} accelerate={accelerate} init={start}: volume {e_vol:.3e} (dev_ref {dev_vol:.3e}, ratio "
          f"{e_vol / dev_vol:.2f}), estimate {e_est:.3e} (dev_ref {dev_est:.3e}, ratio {e_est / dev_est:.2f})")
    assert e_vol <= MARGIN * dev_vol and e_est <= MARGIN * dev_est
    assert not np.isnan(vol).any() and (bits(vol[0, list(z[f"n{ns}/zeroed"])]) == 0).all()
    assert np.array_equal(bits(vol), bits(host(again[0]))) and np.array_equal(bits(est), bits(host(again[2]))), "two calls, one result"
    assert out[3] == again[3], "and one trace"
    assert np.array_equal(host(img), z["img"]) and np.array_equal(host(OTF), z["OTF"]), "inputs are left alone"
    assert np.array_equal(bits(host(mu)), bits(mu_h)) and np.array_equal(bits(host(sd)), bits(sd_h))
    assert init is None or np.array_equal(bits(host(init)), bits(init_h))
    # the objective: one float per iteration, the float64 restatement's within the same margin
    trace, want = out[3], r64[5]
    assert isinstance(trace, list) and len(trace) == N_IT == len(want) and all(type(v) is float for v in trace)
    e_tr = max(abs(a - b) / abs(b) for a, b in zip(trace, want))
    print(f"    objective {e_tr:.3e} relative (ratio {e_tr / max(dev_vol, dev_est):.2f})")
    assert e_tr <= MARGIN * max(dev_vol, dev_est)
    # the prior is in it: far from what the call without one returns
    plain = host(U.XLFMDeconv(OTF, img, N_IT, n_split_fourier=ns, accelerate=accelerate, **deconv_args(z))[0])
    far = float(np.abs(vol.astype(np.float64) - plain).max() / np.abs(plain).max())
    print(f"    {far:.2f} of the plain call's maximum away from the plain call")
    assert far >= 0.1
    if not accelerate:
        rise = max((q - p) / abs(p) for p, q in zip(trace, trace[1:]))
        print(f"    largest relative rise of the objective {rise:.3e}")
        assert rise <= MARGIN * max(dev_vol, dev_est)
    # the objective rides along without touching the result
    quiet = U.XLFMDeconv(OTF, img, N_IT, **dict(kw, trace=False))
    assert quiet[3] == [] and np.array_equal(bits(host(quiet[0])), bits(vol)) and np.array_equal(bits(host(quiet[2])), bits(est))


@pytest.mark.parametrize("accelerate", [False, True], ids=["plain", "accel"])
@pytest.mark.parametrize("name,ns", CASES)
def test_neutral_settings_give_the_plain_call(name, ns, accelerate):
    from cwfa_amd import utils as U
    z = rl(name)
    mu_h, sd_h, _ = prior_of(name, ns)
    OTF, img, mu = dev(z["OTF"]), dev(z["img"]), dev(mu_h)
    sd = dev(np.where(np.isinf(sd_h), f32(1), sd_h))
    base = dict(n_split_fourier=ns, accelerate=accelerate, trace=True, **deconv_args(z))
    want = U.XLFMDeconv(OTF, img, N_IT, **base)
    neutral = {"prior_weight = 0": dict(prior_mean=mu, prior_std=sd, prior_weight=0.0),
               "prior_std = inf": dict(prior_mean=mu, prior_std=torch.full_like(mu, np.inf)),
               "init = ones": dict(init=torch.ones_like(mu)),
               "the defaults": dict(prior_mean=None, prior_std=None, prior_weight=1.0, init=None)}
    for what, kw in neutral.items():
        got = U.XLFMDeconv(OTF, img, N_IT, **base, **kw)
        assert np.array_equal(bits(host(got[0])), bits(host(want[0]))) and np.array_equal(bits(host(got[2])), bits(host(want[2]))), what
        assert got[3] == want[3] and got[4:] == want[4:], what + ": and a penalty of exactly 0"


@pytest.mark.parametrize("accelerate", [False, True], ids=["plain", "accel"])
def test_a_strong_prior_in_the_loop(accelerate):
    """Constant w = 1e6 (sigma = 1e-3) on fixture i: the loop path at a large w.  Against the float64 restatement within 8 dev_ref, and
    no voxel further from the mean than the stationarity identity x - mu = (a / x - 1) / w allows with the float64 loop's last a."""
    from cwfa_amd import utils as U
    z = rl("i")
    mu_h = prior_of("i", 1)[2]                                                           # max(mu, 1e-3 xs): positive everywhere
    sd_h = np.full_like(mu_h, 1e-3)
    kw, keep = dict(accelerate=accelerate, prior_mean=torch.from_numpy(mu_h.copy()), prior_std=torch.from_numpy(sd_h)), {}
    r64 = M.xlfm_deconv_map(*fixture_args("i", 1), torch.float64, keep=keep, **kw)
    r32 = M.xlfm_deconv_map(*fixture_args("i", 1), torch.float32, **kw)
    dev_vol, dev_est = rel(r32[0].numpy(), r64[0].numpy()), rel(r32[1].numpy(), r64[1].numpy())
    assert dev_vol <= 2e-5 and dev_est <= 2e-5
    out = U.XLFMDeconv(dev(z["OTF"]), dev(z["img"]), N_IT, accelerate=accelerate, prior_mean=dev(mu_h), prior_std=dev(sd_h), **deconv_args(z))
    vol, est = host(out[0]), host(out[2])
    e_vol, e_est = rel(vol, r64[0].numpy()), rel(est, r64[1].numpy())
    print(f"w = 1e6: volume {e_vol:.3e} (dev_ref {dev_vol:.3e}, ratio {e_vol / dev_vol:.2f}), estimate {e_est:.3e} (dev_ref {dev_est:.3e}, "
          f"ratio {e_est / dev_est:.2f})")
    assert e_vol <= MARGIN * dev_vol and e_est <= MARGIN * dev_est
    live = [d for d in range(mu_h.shape[1]) if d not in list(z["n1/zeroed"])]
    x64, a64, mu64 = r64[0][:, live].numpy(), keep["a"][:, live].numpy(), mu_h[:, live].astype(np.float64)
    w64 = 1.0 / (sd_h[:, live] * sd_h[:, live]).astype(np.float64)                       # sigma^2 as the loop forms it, in fp32
    allowed = (np.abs(a64 / x64 - 1) / w64).max() / mu64.max()
    err = np.abs(vol[:, live] - mu64).max() / mu64.max()
    print(f"    {err:.3e} of the mean's maximum from the mean; the identity allows {allowed:.3e}")
    assert err <= allowed + MARGIN * dev_vol


def test_tolerance_acts_on_the_objective():
    from cwfa_amd import utils as U
    OTF64, img64 = A.synthetic_problem()
    plain = A.xlfm_deconv_accel(OTF64, img64, N_IT, [16, 16], [16, 16, 6], dtype=torch.float64, accelerate=False)[0]
    mu_h, sd_h, _ = M.prior_recipe(plain.numpy())
    OTF, img, mu, sd = dev(OTF64.to(torch.complex64).numpy()), dev(img64.float().numpy()), dev(mu_h), dev(sd_h)
    kw = dict(ObjSize=[16, 16], PSFShape=[32, 32], ROIsize=[16, 16, 6], prior_mean=mu, prior_std=sd)
    tol, every, n_max = 1e-4, 5, 200
    out = U.XLFMDeconv(OTF, img, n_max, trace=True, tol=tol, check_every=every, **kw)
    tr = out[3]
    n = len(tr)
    print(f"stopped after {n} of {n_max} iterations")
    assert 2 * every <= n < n_max and n % every == 0
    checks = [tr[k] for k in range(every - 1, n, every)]
    drops = [(p - q) / abs(q) for p, q in zip(checks, checks[1:])]
    assert drops[-1] < tol and all(v >= tol for v in drops[:-1]), "the first check that falls below tol ends the loop"
    same = U.XLFMDeconv(OTF, img, n, trace=True, **kw)                                  # the iteration that stops is completed
    assert same[3] == tr and np.array_equal(bits(host(same[0])), bits(host(out[0]))) and np.array_equal(bits(host(same[2])), bits(host(out[2])))
    bare = U.XLFMDeconv(OTF, img, 1, trace=True, ObjSize=[16, 16], PSFShape=[32, 32], ROIsize=[16, 16, 6])
    assert tr[0] > bare[3][0], "the objective at the start holds the penalty of the ones"
    quiet = U.XLFMDeconv(OTF, img, n_max, tol=tol, check_every=every, **kw)
    assert quiet[3] == [] and np.array_equal(bits(host(quiet[0])), bits(host(out[0]))), "tol alone returns no list"


def test_xlfm_deconv_refuses_bad_priors_on_the_device():
    from cwfa_amd import utils as U
    OTF64, img64 = A.synthetic_problem()
    OTF, img = dev(OTF64.to(torch.complex64).numpy()), dev(img64.float().numpy())
    kw = dict(ObjSize=[16, 16], PSFShape=[32, 32], ROIsize=[16, 16, 6])
    one = torch.ones(1, 6, 16, 16, device="cuda")
    run = lambda **more: U.XLFMDeconv(OTF, img, 2, **kw, **more)
    for bad in (one[:, :5], one[..., :15], one[0], one.double()):
        with pytest.raises(ValueError, match="prior_mean must be a float32 tensor"):
            run(prior_mean=bad, prior_std=one)
        with pytest.raises(ValueError, match="prior_std must be a float32 tensor"):
            run(prior_mean=one, prior_std=bad)
        with pytest.raises(ValueError, match="init must be a float32 tensor"):
            run(init=bad)
    with pytest.raises(ValueError, match="together"):
        run(prior_mean=one)
    with pytest.raises(ValueError, match="together"):
        run(prior_std=one)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run(prior_mean=one.cpu(), prior_std=one)

    def planted(value):
        t = one.clone()
        t[0, 3, 7, 9] = value
        return t

    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="prior_std is not > 0"):
            run(prior_mean=one, prior_std=planted(bad))
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="prior_mean is not finite"):
            run(prior_mean=planted(bad), prior_std=one)
    for bad in (-1e-30, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="init is not finite and >= 0"):
            run(init=planted(bad))
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="prior_weight"):
            run(prior_mean=one, prior_std=one, prior_weight=bad)
    # the two bounds, one case on each side: w = 2^60 and w |mu| = 2^60 run and stay finite, the next power of four does not
    ok = run(prior_mean=one, prior_std=planted(2.0 ** -30), trace=True)
    assert torch.isfinite(ok[0]).all() and ok[0][0, 3, 7, 9].item() == 1.0 and all(np.isfinite(ok[3]))
    with pytest.raises(ValueError, match=r"prior_std\^2 exceeds 2\^60"):
        run(prior_mean=one, prior_std=planted(2.0 ** -31))
    with pytest.raises(ValueError, match=r"prior_std\^2 exceeds 2\^60"):
        run(prior_mean=one, prior_std=one, prior_weight=2.0 ** 61)
    for sign in (1.0, -1.0):
        ok = run(prior_mean=planted(sign * 2.0 ** 60), prior_std=one, trace=True)
        assert torch.isfinite(ok[0]).all() and all(np.isfinite(ok[3]))
        with pytest.raises(ValueError, match=r"\|prior_mean\| exceeds 2\^60"):
            run(prior_mean=planted(sign * 2.0 ** 61), prior_std=one)
    assert ok[0][0, 3, 7, 9].item() < 1e-12, "a mean of -2^60 at w = 1 pins the voxel next to 0"
    # valid on both sides of zero, and an init without a prior
    ok = run(prior_mean=-one, prior_std=one, init=planted(0.0), accelerate=True)
    assert torch.isfinite(ok[0]).all()
