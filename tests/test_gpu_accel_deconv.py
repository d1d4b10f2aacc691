"""GPU: the accelerated Richardson-Lucy loop and its convergence trace.

Each new kernel of csrc/deconv_ops.hip alone against numpy, with the bound its arithmetic gives:
  update_accel   x_new and g exact (one fp32 product, one fp32 difference, emulated operation by operation); the two sums against
                 float64 sums of the products (fp32 x fp32 is exact in float64) within n 2^-53 sum|terms|, the bound of any order of n
                 float64 additions;
  alpha          the clamped quotient rounded to fp32; 0 for a zero denominator, a negative quotient, NaN; alpha_max above it;
  predict        exact (difference, product, sum and maximum, each one fp32 operation);
  poisson_nll    within n 2^-53 sum|terms| of the float64 sum of the float64 terms.
Then XLFMDeconv(accelerate=True) on the fixtures recorded from the reference (tests/golden/g25_deconv_rl_*.npz) against the float64
restatement tests/accel_deconv_ref.py: max|gpu - f64| <= 8 dev_ref_accel max|f64|, dev_ref_accel the fp32 CPU restatement's own
distance from the float64 one on the same inputs (computed here, itself <= 2e-5), 8 the margin of tests/test_gpu_deconv.py."""
import functools

import numpy as np
import pytest
import torch

import accel_deconv_ref as A
import deconv_ref as R
from test_deconv_cpu import RL, rel, rl
from test_gpu_deconv import bits, deconv_args, dev, host

pytestmark = pytest.mark.gpu
MARGIN = 8.0
N_IT = 8
# (F, obj, D, depths per launch): element by element with the slab accumulated over chunks of 2 + 1 depths; 16-byte groups; two
# blocks per depth, the second one ragged (72 * 18 = 1296 groups of 1024 per block)
SHAPES = [(9, 5, 3, 2), (16, 8, 3, 3), (96, 72, 2, 2)]


def relu_keep_nan(s):
    return np.where(s > 0, s, np.where(np.isnan(s), s, np.float32(0)))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("F,obj,D,chunk", SHAPES)
def test_update_accel_alpha_predict(F, obj, D, chunk):
    from cwfa_amd import ops
    rng = np.random.default_rng(F + obj)
    po = (F - obj) // 2
    win = (slice(None), slice(None), slice(po, po + obj), slice(po, po + obj))
    y_h = np.zeros((1, D, F, F), dtype=np.float32)
    y_h[win] = np.abs(rng.standard_normal((1, D, obj, obj))).astype(np.float32)
    y_h[0, 0, po, po], y_h[0, D - 1, po + obj - 1, po + obj - 1] = 0.0, 0.0
    b_h = (1 + 0.3 * rng.standard_normal((1, D, F, F))).astype(np.float32)
    idx = R.np_shift_index(F)
    inside = np.zeros((F, F), dtype=bool)
    inside[np.ix_(idx[po:po + obj], idx[po:po + obj])] = True
    b_h[:, :, ~inside] = np.nan                                                          # whatever lies outside the window is not used
    m_h = b_h[:, :, idx][:, :, :, idx][win]
    xn_want = y_h[win] * m_h
    g_want = xn_want - y_h[win]
    gp_h = (np.float32(2) * g_want + 0.1 * rng.standard_normal(g_want.shape).astype(np.float32)).astype(np.float32)   # quotient near 0.5
    xp_h = np.abs(rng.standard_normal(g_want.shape)).astype(np.float32)
    xp_h[0, 0, 0, :2] = xn_want[0, 0, 0, :2] + np.float32(8)                            # a prediction below zero

    y, b, g, xn, xp = dev(y_h), dev(b_h), dev(gp_h), torch.full((1, D, obj, obj), np.nan, device="cuda"), dev(xp_h)
    slab = ops.deconv_accel_slab(chunk, obj, "cuda")
    assert slab.shape == (chunk * -(-obj * obj // 1024), 2) and not slab.any()
    for jj in range(0, D, chunk):
        ops.deconv_update_accel(y[:, jj:jj + chunk], b[:, jj:jj + chunk], g[:, jj:jj + chunk], xn[:, jj:jj + chunk], slab, obj, po)
    assert np.array_equal(bits(host(xn)), bits(xn_want)), "the single fp32 product of deconv_update"
    assert np.array_equal(bits(host(g)), bits(g_want)), "one fp32 difference, written over the previous step"
    assert np.array_equal(bits(host(y)), bits(y_h)) and np.array_equal(bits(host(b)), bits(b_h)), "inputs are only read"
    plain = ops.deconv_update(dev(y_h), dev(np.nan_to_num(b_h)), obj, po)
    assert np.array_equal(bits(host(plain)[win]), bits(host(xn)))

    n = D * obj * obj
    t_num, t_den = g_want.astype(np.float64) * gp_h.astype(np.float64), gp_h.astype(np.float64) ** 2
    s_h = host(slab)
    e_num, e_den = abs(s_h[:, 0].sum() - t_num.sum()), abs(s_h[:, 1].sum() - t_den.sum())
    b_num, b_den = n * 2.0 ** -53 * np.abs(t_num).sum(), n * 2.0 ** -53 * t_den.sum()
    print(f"F={F} obj={obj}: sum g g_prev off by {e_num:.3e} (bound {b_num:.3e}), sum g_prev^2 by {e_den:.3e} (bound {b_den:.3e})")
    assert e_num <= b_num and e_den <= b_den
    if D > chunk:
        assert s_h.shape[0] == chunk < D, "one row per depth of a chunk: the second chunk added to the rows of the first"

    alpha = torch.full((1,), np.nan, device="cuda")
    ops.deconv_alpha(slab, 0.999, alpha)
    q = t_num.sum() / t_den.sum()
    a_h = host(alpha)[0]
    assert 0.3 < q < 0.7 and a_h.dtype == np.float32
    # the quotient of two sums each within its bound, rounded once to fp32
    assert abs(float(a_h) - q) <= q * (2.0 ** -24 + b_num / abs(t_num.sum()) + b_den / t_den.sum() + 2.0 ** -52)
    assert not slab.any(), "the slab is zeroed for the next iteration"

    ops.deconv_predict(y, xn, xp, alpha, obj, po)
    with np.errstate(invalid="ignore"):
        want = relu_keep_nan(xn_want + a_h * (xn_want - xp_h))                            # three fp32 operations, then the maximum
    got = host(y)
    assert (want == 0).sum() >= 2 and (want > 0).sum() > want.size // 2
    assert np.array_equal(bits(got[win]), bits(want))
    border = np.ones((F, F), dtype=bool)
    border[po:po + obj, po:po + obj] = False
    assert (bits(got[:, :, border]) == 0).all(), "the border stays exactly +0.0"
    assert np.array_equal(bits(host(xn)), bits(xn_want)) and np.array_equal(bits(host(xp)), bits(xp_h))


def test_alpha_edge_cases():
    from cwfa_amd import ops
    rows = 2500                                                                          # more rows than the block has threads

    def run(num, den, alpha_max=0.999):
        s = np.zeros((rows, 2))
        s[:, 0], s[:, 1] = num, den
        slab, alpha = dev(s), torch.full((1,), np.nan, device="cuda")
        ops.deconv_alpha(slab, alpha_max, alpha)
        assert not slab.any()
        return host(alpha)[0]

    assert run(0.25, 1.0) == np.float32(0.25) and run(1.0, 3.0) == np.float32(1.0 / 3.0)
    assert run(1.0, 0.0) == 0 and run(0.0, 0.0) == 0 and run(-1.0, 0.0) == 0, "zero denominator: no previous step"
    assert run(-1.0, 2.0) == 0, "negative quotient"
    assert run(3.0, 2.0) == np.float32(0.999) and run(3.0, 2.0, 0.5) == np.float32(0.5) and run(3.0, 2.0, 0.0) == 0, "above alpha_max"
    assert run(np.nan, 1.0) == 0 and run(1.0, np.nan) == 0 and run(np.inf, 1.0) == 0 and run(np.inf, np.inf) == 0, "not finite"
    part = np.zeros(rows)
    part[1300] = np.nan                                                                  # one bad partial anywhere
    assert run(part, 1.0) == 0
    with pytest.raises(RuntimeError, match="alpha_max"):
        ops.deconv_alpha(torch.zeros(4, 2, dtype=torch.float64, device="cuda"), 1.0, torch.zeros(1, device="cuda"))


@pytest.mark.parametrize("n", [1003, 4096, 300001])
def test_poisson_nll(n):
    """1003 and 300001 element by element, 4096 in 16-byte groups; 300001 elements are more blocks than the workspace holds
    partials for, so every thread walks the grid stride."""
    from cwfa_amd import ops
    rng = np.random.default_rng(n)
    est_h = (np.abs(rng.standard_normal(n)) * 30).astype(np.float32)
    img_h = rng.poisson(est_h + 1).astype(np.float32)
    est_h[::11], img_h[::7] = 0.0, 0.0
    trace = torch.full((5,), -7.0, dtype=torch.float64, device="cuda")
    ops.deconv_poisson_nll(dev(img_h), dev(est_h), trace, 3)
    e, a = est_h.astype(np.float64), img_h.astype(np.float64)
    terms = e - a * np.log(e + 1e-8)
    got = host(trace)
    err, bound = abs(got[3] - terms.sum()), n * 2.0 ** -53 * np.abs(terms).sum()
    print(f"n={n}: NLL {got[3]:.6f} off by {err:.3e} (bound {bound:.3e})")
    assert err <= bound and (got[[0, 1, 2, 4]] == -7.0).all(), "one element of the trace is written"
    ws = torch.empty(8192, dtype=torch.uint8, device="cuda")
    ops.deconv_poisson_nll(dev(img_h), dev(est_h), trace, 0, ws)
    assert host(trace)[0] == got[3], "bitwise repeatable"
    with pytest.raises(ValueError, match="trace"):
        ops.deconv_poisson_nll(dev(img_h), dev(est_h), trace, 5)
    with pytest.raises(ValueError, match="workspace"):
        ops.deconv_poisson_nll(dev(img_h), dev(est_h), trace, 0, ws[:100])


def test_wrappers_refuse_wrong_tensors():
    from cwfa_amd import ops
    o, w = torch.zeros(1, 2, 16, 16, device="cuda"), torch.zeros(1, 2, 8, 8, device="cuda")
    slab, alpha = ops.deconv_accel_slab(2, 8, "cuda"), torch.zeros(1, device="cuda")
    with pytest.raises(ValueError, match="windows"):
        ops.deconv_update_accel(o, o.clone(), w[:, :1], w.clone(), slab, 8, 4)
    with pytest.raises(ValueError, match="one shape"):
        ops.deconv_update_accel(o, o[:, :1].clone(), w, w.clone(), slab, 8, 4)
    with pytest.raises(ValueError, match="slab"):
        ops.deconv_update_accel(o, o.clone(), w, w.clone(), slab.float(), 8, 4)
    with pytest.raises(RuntimeError, match="rows"):
        ops.deconv_update_accel(o, o.clone(), w, w.clone(), slab[:1], 8, 4)
    with pytest.raises(RuntimeError, match="share no buffer"):
        ops.deconv_update_accel(o, o.clone(), w, w, slab, 8, 4)
    with pytest.raises(TypeError, match="float32"):
        ops.deconv_predict(o, w.double(), w, alpha, 8, 4)
    with pytest.raises(ValueError, match="windows"):
        ops.deconv_predict(o, w, w[:, :1], alpha, 8, 4)
    with pytest.raises(ValueError, match="alpha"):
        ops.deconv_predict(o, w, w.clone(), alpha.double(), 8, 4)
    with pytest.raises(ValueError, match="contiguous"):
        ops.deconv_predict(o, w, w.clone().transpose(2, 3), alpha, 8, 4)
    with pytest.raises(ValueError, match="differ in size"):
        ops.deconv_poisson_nll(o, w, torch.zeros(2, dtype=torch.float64, device="cuda"), 0)
    with pytest.raises(ValueError, match="float64"):
        ops.deconv_poisson_nll(o, o.clone(), torch.zeros(2, device="cuda"), 0)


def test_accel_offsets_beyond_2_31_elements():
    """One launch of update_accel and one of predict over 130 planes of 4096 x 4096 (2^31 + 2^25 floats), zero except in the last
    plane, where a 32-bit offset would wrap to the front."""
    from cwfa_amd import ops
    D, S, obj, po = 130, 4096, 2048, 1024
    last = torch.randn(S, S, device="cuda")
    want_m = R.shift(last[None, None])[0, 0, po:po + obj, po:po + obj]
    obj_pad, b = torch.zeros(1, D, S, S, device="cuda"), torch.zeros(1, D, S, S, device="cuda")
    obj_pad[0, D - 1, po:po + obj, po:po + obj] = 2.0
    b[0, D - 1] = last
    g, xn, xp = (torch.zeros(1, D, obj, obj, device="cuda") for _ in range(3))
    g[0, D - 1] = torch.randn(obj, obj, device="cuda")
    gp = g[0, D - 1].clone()
    xp[0, D - 1] = 1.0
    slab, alpha = ops.deconv_accel_slab(D, obj, "cuda"), torch.full((1,), 0.5, device="cuda")
    ops.deconv_update_accel(obj_pad, b, g, xn, slab, obj, po)
    x_want = 2.0 * want_m
    assert torch.equal(xn[0, D - 1], x_want) and torch.equal(g[0, D - 1], x_want - 2.0)
    assert not xn[0, :D - 1].any() and not g[0, :D - 1].any(), "nothing wrapped to the front"
    num, den = (g[0, D - 1].double() * gp.double()).sum().item(), (gp.double() ** 2).sum().item()
    got = slab.sum(0).tolist()
    assert abs(got[0] - num) <= 1e-9 * abs(den) and abs(got[1] - den) <= 1e-9 * den
    ops.deconv_predict(obj_pad, xn, xp, alpha, obj, po)
    y_want = torch.relu(x_want + 0.5 * (x_want - 1.0))
    assert torch.equal(obj_pad[0, D - 1, po:po + obj, po:po + obj], y_want) and (y_want > 0).any() and (y_want == 0).any()
    assert not obj_pad[0, :D - 1].any(), "nothing wrapped to the front"
    obj_pad[0, D - 1, po:po + obj, po:po + obj] = 0
    assert not obj_pad[0, D - 1].any(), "the border of the last plane stays 0"


# ------------------------------------------------------------------------------------------------ XLFMDeconv on the fixtures
@functools.lru_cache(maxsize=None)
def restated(name, ns, accelerate=True):
    """The float64 restatement on a fixture's inputs and the fp32 CPU restatement's distance from it: computed once, shared."""
    z = rl(name)
    args = (torch.from_numpy(z["OTF"]), torch.from_numpy(z["img"]), N_IT, [int(v) for v in z["ObjSize"]], [int(v) for v in z["ROIsize"]], ns,
            int(z["mult"]))
    r64 = A.xlfm_deconv_accel(*args, torch.float64, accelerate=accelerate)
    r32 = A.xlfm_deconv_accel(*args, torch.float32, accelerate=accelerate)
    assert r64[4] == r32[4] == N_IT
    return r64, rel(r32[0].numpy(), r64[0].numpy()), rel(r32[1].numpy(), r64[1].numpy())


CASES = [(n, s) for n in RL for s in RL[n]]


@pytest.mark.parametrize("name,ns", CASES)
def test_accelerated_deconv_matches_the_float64_restatement(name, ns):
    from cwfa_amd import utils as U
    z = rl(name)
    r64, dev_vol, dev_est = restated(name, ns)
    assert dev_vol <= 2e-5 and dev_est <= 2e-5, "the yardstick's own fp32 distance"
    OTF, img = dev(z["OTF"]), dev(z["img"])
    kw = dict(n_split_fourier=ns, accelerate=True, trace=True, **deconv_args(z))
    out = U.XLFMDeconv(OTF, img, N_IT, **kw)
    again = U.XLFMDeconv(OTF, img, N_IT, **kw)
    assert len(out) == 6 and out[1] == 0 and out[4] == r64[2] and out[5] == r64[3]
    vol, est = host(out[0]), host(out[2])
    assert vol.shape == tuple(r64[0].shape) and est.shape == tuple(r64[1].shape)
    e_vol, e_est = rel(vol, r64[0].numpy()), rel(est, r64[1].numpy())
    print(f"{name} n_split_fourier={ns}: volume {e_vol:.3e} (dev_ref_accel {dev_vol:.3e}, ratio {e_vol / dev_vol:.2f}), "
          f"estimate {e_est:.3e} (dev_ref_accel {dev_est:.3e}, ratio {e_est / dev_est:.2f})")
    assert e_vol <= MARGIN * dev_vol and e_est <= MARGIN * dev_est
    assert (bits(vol[0, list(z[f"n{ns}/zeroed"])]) == 0).all()
    assert np.array_equal(bits(vol), bits(host(again[0]))) and np.array_equal(bits(est), bits(host(again[2]))), "two calls, one result"
    assert out[3] == again[3], "and one trace"
    assert np.array_equal(host(img), z["img"]) and np.array_equal(host(OTF), z["OTF"]), "inputs are left alone"
    # the trace: one float per iteration, the float64 restatement's within the same margin
    trace, want = out[3], r64[5]
    assert isinstance(trace, list) and len(trace) == N_IT == len(want) and all(type(v) is float for v in trace)
    e_tr = max(abs(a - b) / abs(b) for a, b in zip(trace, want))
    print(f"{name} n_split_fourier={ns}: trace {e_tr:.3e} relative")
    assert e_tr <= MARGIN * max(dev_vol, dev_est)


@pytest.mark.parametrize("name,ns", CASES)
def test_new_arguments_at_their_defaults_change_nothing(name, ns):
    from cwfa_amd import utils as U
    z = rl(name)
    OTF, img = dev(z["OTF"]), dev(z["img"])
    a = U.XLFMDeconv(OTF, img, int(z["nIt"]), n_split_fourier=ns, **deconv_args(z))
    b = U.XLFMDeconv(OTF, img, int(z["nIt"]), n_split_fourier=ns, accelerate=False, trace=False, tol=None, **deconv_args(z))
    assert a[3] == [] and b[3] == [] and a[1] == b[1] == 0 and a[4:] == b[4:]
    assert np.array_equal(bits(host(a[0])), bits(host(b[0]))) and np.array_equal(bits(host(a[2])), bits(host(b[2])))
    # the trace rides along without touching the result, and the plain loop's likelihood does not rise
    c = U.XLFMDeconv(OTF, img, N_IT, n_split_fourier=ns, trace=True, **deconv_args(z))
    d = U.XLFMDeconv(OTF, img, N_IT, n_split_fourier=ns, **deconv_args(z))
    assert np.array_equal(bits(host(c[0])), bits(host(d[0]))) and np.array_equal(bits(host(c[2])), bits(host(d[2])))
    r64, dev_vol, dev_est = restated(name, ns, accelerate=False)
    tr = c[3]
    assert len(tr) == N_IT and max(abs(p - q) / abs(q) for p, q in zip(tr, r64[5])) <= MARGIN * max(dev_vol, dev_est)
    rise = max((q - p) / abs(p) for p, q in zip(tr, tr[1:]))
    print(f"{name} n_split_fourier={ns}: largest relative rise of the plain loop's likelihood {rise:.3e}")
    assert rise <= MARGIN * max(dev_vol, dev_est)


def test_tolerance_stops_early_and_the_trace_says_where():
    from cwfa_amd import utils as U
    OTF64, img64 = A.synthetic_problem()
    OTF, img = dev(OTF64.to(torch.complex64).numpy()), dev(img64.float().numpy())
    kw = dict(ObjSize=[16, 16], PSFShape=[32, 32], ROIsize=[16, 16, 6], accelerate=True)
    tol, every, n_max = 1e-4, 5, 60
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
    quiet = U.XLFMDeconv(OTF, img, n_max, tol=tol, check_every=every, **kw)
    assert quiet[3] == [] and np.array_equal(bits(host(quiet[0])), bits(host(out[0]))), "tol alone returns no list"
    r64 = A.xlfm_deconv_accel(OTF64, img64, n, [16, 16], [16, 16, 6], dtype=torch.float64)
    r32 = A.xlfm_deconv_accel(OTF64, img64, n, [16, 16], [16, 16, 6], dtype=torch.float32)
    e_vol, dev_vol = rel(host(out[0]), r64[0].numpy()), rel(r32[0].numpy(), r64[0].numpy())
    print(f"volume after {n} accelerated iterations {e_vol:.3e} (dev_ref_accel {dev_vol:.3e})")
    assert e_vol <= MARGIN * dev_vol, "and the volume is the accelerated loop's"
