"""CPU: MAP Richardson-Lucy without a GPU -- the restatement tests/map_deconv_ref.py against
tests/accel_deconv_ref.py (bit-equal in float32 with no prior, with w = 0 and with sigma = inf), the M-step's stationarity and special
values, the descent of the objective on the four fixtures, ``prior_from_posterior``, the argument validation of the three new entry
points through the built library, and the refusals XLFMDeconv decides before any device work."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import accel_deconv_ref as A
import map_deconv_ref as M
from test_deconv_cpu import RL, rl

N_IT = 8


@pytest.fixture(scope="module")
def L():
    from cwfa_amd import _lib, build
    build.build_all()
    return _lib.lib()


@pytest.fixture(scope="module")
def ptr():
    buf = ctypes.create_string_buffer(16384)
    base = ctypes.addressof(buf)
    return ctypes.c_void_p((base + 15) & ~15)


def fixture_args(name, ns=1, n_it=N_IT):
    z = rl(name)
    return (torch.from_numpy(z["OTF"]), torch.from_numpy(z["img"]), n_it, [int(v) for v in z["ObjSize"]], [int(v) for v in z["ROIsize"]], ns,
            int(z["mult"]))


@functools.lru_cache(maxsize=None)
def fixture_prior(name, ns=1):
    """(mu, sigma, start) of the tests' prior recipe on a fixture: from the plain loop's float64 result after 8 iterations."""
    plain = A.xlfm_deconv_accel(*fixture_args(name, ns), torch.float64, accelerate=False)[0]
    return tuple(torch.from_numpy(v) for v in M.prior_recipe(plain.numpy()))


def same_bits(a, b):
    return np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(RL))
@pytest.mark.parametrize("accelerate", [False, True])
def test_defaults_and_a_zero_prior_are_the_existing_restatement(name, accelerate):
    mu = fixture_prior(name)[0]
    for ns in RL[name]:
        args = fixture_args(name, ns)
        want = A.xlfm_deconv_accel(*args, torch.float32, accelerate=accelerate)
        plain = M.xlfm_deconv_map(*args, torch.float32, accelerate=accelerate)
        assert same_bits(plain[0], want[0]) and same_bits(plain[1], want[1]) and plain[2:] == want[2:], "no prior, no init"
        ones = M.xlfm_deconv_map(*args, torch.float32, accelerate=accelerate, init=torch.ones_like(mu))
        assert same_bits(ones[0], want[0]) and same_bits(ones[1], want[1])
        sd = torch.full_like(mu, 0.5)
        zero_w = M.xlfm_deconv_map(*args, torch.float32, accelerate=accelerate, prior_mean=mu, prior_std=sd, prior_weight=0.0)
        no_sd = M.xlfm_deconv_map(*args, torch.float32, accelerate=accelerate, prior_mean=mu, prior_std=torch.full_like(mu, np.inf))
        for got in (zero_w, no_sd):
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), "w = 0: c = 1, r = 1, 2a / 2 = a"
            assert got[5] == want[5] and got[6] == want[6], "and a penalty of exactly 0"


def test_m_step_is_stationary_on_both_branches():
    """float64: w x^2 + c x - a = 0 to rounding.  Each of the three terms is computed with a few roundings, so the residual is a
    few 2^-53 of their largest magnitude."""
    rng = np.random.default_rng(21)
    n = 20000
    a = torch.from_numpy(np.abs(rng.standard_normal(n)) * 10.0 ** rng.uniform(-3, 3, n))
    mu = torch.from_numpy(np.abs(rng.standard_normal(n)) * 10.0 ** rng.uniform(-2, 2, n))
    mu[::5] *= -1                                                                        # a de-normalised mean may be negative
    w =torch.from_numpy(10.0 ** rng.uniform(-4, 4, n))
    x = M.m_step(a, mu, w)
    c = 1 - w * mu
    share = float((c <= 0).double().mean())
    assert 0.25 <= share <= 0.75, share
    assert bool((x > 0).all()) and bool(torch.isfinite(x).all())
    res = (w * x * x + c * x - a).abs()
    size = torch.maximum(torch.maximum(w * x * x, (c * x).abs()), a)
    worst = float((res / size).max())
    print(f"largest residual of the quadratic relative to its largest term: {worst:.3e}, {share:.0%} on the second branch")
    assert worst <= 16 * 2.0 ** -53


def test_m_step_special_values():
    for dt in (torch.float32, torch.float64):
        t = lambda *v: torch.tensor(v, dtype=dt)
        # a = 0: with c > 0 the voxel stays 0; with c < 0 the prior revives it at mu - 1 / w; c == 0 gives 0, not 0 / 0
        got = M.m_step(t(0.0, 0.0, 0.0), t(0.5, 4.0, 2.0), t(1.0, 1.0, 0.5))
        assert got.tolist() == [0.0, 3.0, 0.0] and not torch.isnan(got).any()
        assert float(M.m_step(t(0.0), t(2.5), t(2.0))) == 2.5 - 1 / 2.0, "the revival value mu - 1 / w"
        # c == 0 with a > 0: x = sqrt(a / w)
        assert float(M.m_step(t(8.0), t(2.0), t(0.5))) == 4.0
        # w = 0 is the plain update, also for the a < 0 a back projection's rounding can leave
        a = t(0.0, 1e-30, 3.25, 7e8, -1e-9)
        assert torch.equal(M.m_step(a, t(1.0, -2.0, 3.0, 0.0, 5.0), torch.zeros(5, dtype=dt)), a)
        # a < 0 under a prior: the discriminant is held at 0, nothing is NaN
        neg = M.m_step(t(-1.0, -1.0), t(0.9, 3.0), t(1.0, 1.0))
        assert not torch.isnan(neg).any() and float(neg[1]) > 0
        # a negative mean pulls towards 0 from above: the result stays positive
        assert 0 < float(M.m_step(t(1.0), t(-5.0), t(3.0))) < 1.0


def test_a_strong_prior_returns_its_mean():
    rng = np.random.default_rng(3)
    for dt, eps in ((torch.float32, 2.0 ** -24), (torch.float64, 2.0 ** -53)):
        mu = torch.from_numpy(rng.uniform(1.0, 100.0, 4096)).to(dt)
        a = (mu * torch.from_numpy(rng.uniform(0.5, 2.0, 4096)).to(dt))                  # an update within a factor 2 of the mean
        x = M.m_step(a, mu, torch.full_like(mu, 1e6))
        worst = float(((x - mu).abs() / mu).max())
        print(f"{dt}: w = 1e6 lands within {worst:.3e} of mu")
        # stationarity: x - mu = (a / x - 1) / w, below 1 / w here, so 1e-6 mu for mu >= 1; two roundings of slack
        assert worst <= 1e-6 + 2 * eps


@pytest.mark.parametrize("accelerate", [False, True])
def test_a_strong_prior_in_the_loop_obeys_the_stationarity_identity(accelerate):
    """Constant w = 1e6 (sigma = 1e-3) on fixture i.  In the loop a = y * back projection is not within a factor 2 of the mean, so
    the distance from the mean is not 1e-6 of it; what holds is the identity x - mu = (a / x - 1) / w, in the units of x, with the
    a of the last iteration.  Asserted per voxel in float64, and as the distance it implies in both dtypes."""
    mu32 = fixture_prior("i")[2]                                                        # max(mu, 1e-3 xs): positive everywhere
    keep_d = [d for d in range(mu32.shape[1]) if d not in list(rl("i")["n1/zeroed"])]
    for dt, eps in ((torch.float64, 2.0 ** -53), (torch.float32, 2.0 ** -24)):
        mu, sd, keep = mu32.to(dt), torch.full_like(mu32, 1e-3).to(dt), {}
        x = M.xlfm_deconv_map(*fixture_args("i"), dt, accelerate=accelerate, prior_mean=mu, prior_std=sd, keep=keep)[0][:, keep_d]
        a, mu, w = keep["a"][:, keep_d].double(), mu[:, keep_d].double(), (1 / (sd * sd))[:, keep_d].double()
        x = x.double()
        assert bool((x > 0).all()) and float(w.min()) > 0.99e6
        pull = (a / x - 1).abs() / w                                                     # the identity's right-hand side, per voxel
        err, bound = float((x - mu).abs().max() / mu.max()), float(pull.max() / mu.max())
        print(f"{dt}, accelerate={accelerate}: {err:.3e} of the mean's maximum from the mean; the identity allows {bound:.3e} "
              f"(largest |a / x - 1| {float((a / x - 1).abs().max()):.2f})")
        assert err <= bound + 4 * eps, "no voxel is further from the mean than its own update pulls it"
        if dt is torch.float64:
            assert bool(((x - mu - (a / x - 1) / w).abs() <= 16 * eps * torch.maximum(x, a / (x * w))).all()), "per voxel, to rounding"


@pytest.mark.parametrize("name", list(RL))
def test_the_objective_does_not_rise_in_the_plain_loop(name):
    mu, sd, start = fixture_prior(name)
    branch = float((1.0 / (sd * sd) * mu >= 1).float().mean())
    assert 0.25 <= branch <= 0.45 and 0.05 <= float(torch.isinf(sd).float().mean()) <= 0.15
    for init in (None, start):
        r = M.xlfm_deconv_map(*fixture_args(name), torch.float64, prior_mean=mu, prior_std=sd, init=init)
        tr = r[5]
        drops = [(p - q) / abs(p) for p, q in zip(tr, tr[1:])]
        print(f"{name}, start {'ones' if init is None else 'mu'}: relative falls of the objective {min(drops):.2e} .. {max(drops):.2e}")
        assert len(tr) == N_IT and all(q <= p for p, q in zip(tr, tr[1:]))
    plain = A.xlfm_deconv_accel(*fixture_args(name), torch.float64, accelerate=False)[0]
    keep = [d for d in range(mu.shape[1]) if d not in list(rl(name)["n1/zeroed"])]
    far = float((r[0][:, keep] - plain[:, keep]).abs().max() / plain.abs().max())
    print(f"{name}: the MAP result is {far:.2f} of the plain result's maximum away from it")
    assert far >= 0.1


# ------------------------------------------------------------------------------------------------ the helper
def test_prior_from_posterior_embeds_and_round_trips():
    from cwfa_amd import utils as U
    rng = np.random.default_rng(5)
    for (d, h, w_), (nd, obj) in (((4, 6, 7), (9, 12)), ((5, 5, 8), (5, 9)), ((3, 4, 4), (3, 4))):
        mean = torch.from_numpy(rng.standard_normal((1, d, h, w_)).astype(np.float32))
        mean[0, 0, 0, 0] = -0.0
        std = torch.from_numpy(np.abs(rng.standard_normal((1, d, h, w_))).astype(np.float32) + 0.1)
        pm, ps = U.prior_from_posterior(mean, std, nd, obj)
        assert pm.shape == ps.shape == (1, nd, obj, obj) and pm.dtype == torch.float32
        d0, d1 = U.crop_offsets(nd, d)
        back_m, back_s = U.crop_volume_center(pm[:, d0:d1], mean.shape), U.crop_volume_center(ps[:, d0:d1], mean.shape)
        assert same_bits(back_m.contiguous(), mean) and same_bits(back_s.contiguous(), std), "bit for bit, -0.0 included"
        inside = torch.zeros(1, nd, obj, obj, dtype=torch.bool)
        (h0, h1), (w0, w1) = U.crop_offsets(obj, h), U.crop_offsets(obj, w_)
        inside[:, d0:d1, h0:h1, w0:w1] = True
        assert int(inside.sum()) == mean.numel()
        assert bool((pm[~inside] == 0).all()) and bool(torch.isposinf(ps[~inside]).all()), "outside: mean 0, std +inf"
        sm, ss = U.prior_from_posterior(mean, std, nd, obj, scale=3.0, offset=-0.5)
        assert torch.equal(sm[inside], (mean * 3.0 + -0.5).flatten()) and torch.equal(ss[inside], (std * 3.0).flatten())
        assert bool((sm[~inside] == 0).all()) and bool(torch.isposinf(ss[~inside]).all())
    with pytest.raises(ValueError, match="cannot crop"):
        U.prior_from_posterior(mean, std, 2, 4)
    with pytest.raises(ValueError, match="one shape"):
        U.prior_from_posterior(mean, std[:, :1], 3, 4)


# ------------------------------------------------------------------------------------------------ arguments
def test_update_map_arguments(L, ptr):
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(5)]
    ok = (q[0], q[1], q[2], q[3])
    for k in range(4):
        args = list(ok)
        args[k] = None
        assert L.cwfa_deconv_update_map_f32(*args, q[4], 64, 1, 8, 4, 2, None) == -1 and b"cwfa_deconv_update_map_f32: null" in L.cwfa_last_error()
    assert L.cwfa_deconv_update_map_f32(*ok, q[4], 64, -1, 8, 4, 2, None) == -2 and L.cwfa_deconv_update_map_f32(*ok, q[4], 64, 1, 8, -4, 2, None) == -2
    assert L.cwfa_deconv_update_map_f32(*ok, q[4], 64, 65536, 8, 4, 2, None) == -2 and L.cwfa_deconv_update_map_f32(*ok, q[4], 64, 1, 46341, 4, 2, None) == -2
    for obj, po in ((4, 5), (4, -1), (9, 0)):
        assert L.cwfa_deconv_update_map_f32(*ok, q[4], 64, 1, 8, obj, po, None) == -1 and b"not inside" in L.cwfa_last_error()
    assert L.cwfa_deconv_update_map_f32(q[0], q[0], q[2], q[3], q[4], 64, 1, 8, 4, 2, None) == -1 and b"same tensor" in L.cwfa_last_error()
    for bad in ((q[0], q[1], q[0], q[3]), (q[0], q[1], q[2], q[0])):
        assert L.cwfa_deconv_update_map_f32(*bad, q[4], 64, 1, 8, 4, 2, None) == -1 and b"shares no buffer" in L.cwfa_last_error(), bad
    assert L.cwfa_deconv_update_map_f32(*ok, ctypes.c_void_p(q[4].value + 4), 64, 1, 8, 4, 2, None) == -3 and b"8-byte" in L.cwfa_last_error()
    # 3 depths of a 40 x 40 window: 400 sixteen-byte groups are two blocks of 256 each, 1600 elements (an odd offset) seven
    assert L.cwfa_deconv_update_map_f32(*ok, q[4], 5, 3, 48, 40, 4, None) == -1 and b"need 6" in L.cwfa_last_error()
    assert L.cwfa_deconv_update_map_f32(*ok, q[4], 20, 3, 46, 40, 3, None) == -1 and b"need 21" in L.cwfa_last_error()
    assert L.cwfa_deconv_update_map_f32(*ok, q[4], 0, 0, 8, 4, 2, None) == 0 and L.cwfa_deconv_update_map_f32(*ok, q[4], 0, 1, 8, 0, 2, None) == 0
    assert L.cwfa_deconv_update_map_f32(*ok, None, 0, 0, 8, 4, 2, None) == 0, "no penalty slab is allowed"


def test_update_accel_map_arguments(L, ptr):
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(9)]
    ok = tuple(q[:8])                                    # obj_pad, b, g_prev, mu, w, x_new, g, slab
    call = lambda a, rows=64, pen=q[8], pen_rows=64, shape=(1, 8, 4, 2): L.cwfa_deconv_update_accel_map_f32(*a, rows, pen, pen_rows, *shape, None)
    for k in range(8):
        args = list(ok)
        args[k] = None
        assert call(args) == -1 and b"cwfa_deconv_update_accel_map_f32: null" in L.cwfa_last_error()
    assert call(ok, shape=(-1, 8, 4, 2)) == -2 and call(ok, shape=(1, 8, -4, 2)) == -2
    assert call(ok, shape=(65536, 8, 4, 2)) == -2 and call(ok, shape=(1, 46341, 4, 2)) == -2
    for po in (5, -1):
        assert call(ok, shape=(1, 8, 4, po)) == -1 and b"not inside" in L.cwfa_last_error()
    same = list(ok)
    same[1] = q[0]
    assert call(same) == -1 and b"same tensor" in L.cwfa_last_error()
    for out, src in ((5, 6), (5, 2), (5, 0), (5, 1), (5, 3), (5, 4), (6, 0), (6, 1), (6, 3), (6, 4)):
        args = list(ok)
        args[out] = q[src]
        assert call(args) == -1 and b"share no buffer" in L.cwfa_last_error(), (out, src)
    odd = list(ok)
    odd[7] = ctypes.c_void_p(q[7].value + 4)
    assert call(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    assert call(ok, pen=ctypes.c_void_p(q[8].value + 4)) == -3
    assert call(ok, pen=q[7]) == -1 and b"same buffer" in L.cwfa_last_error()
    assert call(ok, rows=2, shape=(3, 48, 40, 4)) == -1 and b"the slab holds 2 rows, 3 depths need 3" in L.cwfa_last_error()
    assert call(ok, pen_rows=5, shape=(3, 46, 40, 3)) == -1 and b"the penalty slab holds 5 rows, 3 depths need 6" in L.cwfa_last_error()
    assert call(ok, rows=0, pen_rows=0, shape=(0, 8, 4, 2)) == 0 and call(ok, rows=0, pen_rows=0, shape=(1, 8, 0, 2)) == 0
    assert call(ok, rows=0, pen=None, pen_rows=0, shape=(0, 8, 4, 2)) == 0, "no penalty slab is allowed"
    inplace = list(ok)
    inplace[6] = q[2]
    assert call(inplace, rows=0, pen_rows=0, shape=(0, 8, 4, 2)) == 0, "g == g_prev is allowed"


def test_penalty_arguments(L, ptr):
    p, q = ptr, ctypes.c_void_p(ptr.value + 1024)
    assert L.cwfa_deconv_penalty_f64(None, 4, q, 0, 4, None) == -1 and b"cwfa_deconv_penalty_f64: null" in L.cwfa_last_error()
    assert L.cwfa_deconv_penalty_f64(p, 4, None, 0, 4, None) == -1
    assert L.cwfa_deconv_penalty_f64(p, -1, q, 0, 4, None) == -2
    for index, length in ((4, 4), (-1, 4), (0, 0)):
        assert L.cwfa_deconv_penalty_f64(p, 4, q, index, length, None) == -1 and b"not inside a trace" in L.cwfa_last_error()
    assert L.cwfa_deconv_penalty_f64(ctypes.c_void_p(p.value + 4), 4, q, 0, 4, None) == -3
    assert L.cwfa_deconv_penalty_f64(p, 4, ctypes.c_void_p(q.value + 4), 0, 4, None) == -3
    assert L.cwfa_deconv_penalty_f64(p, 4, p, 0, 4, None) == -1 and b"same buffer" in L.cwfa_last_error()
    assert L.cwfa_deconv_penalty_f64(p, 0, q, 0, 4, None) == 0


def test_xlfm_deconv_refuses_bad_prior_arguments_before_any_device_work():
    from cwfa_amd import ops, utils as U
    otf = torch.zeros(1, 3, 36, 19, dtype=torch.complex64)
    img = torch.ones(1, 1, 24, 24)
    v = torch.ones(1, 3, 12, 12)
    run = lambda **kw: U.XLFMDeconv(otf, img, 2, ObjSize=[12, 12], **kw)
    with pytest.raises(ValueError, match="together"):
        run(prior_mean=v)
    with pytest.raises(ValueError, match="together"):
        run(prior_std=v)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="prior_weight"):
            run(prior_mean=v, prior_std=v, prior_weight=bad)
    for name in ("prior_mean", "prior_std", "init"):
        for bad in (v[:, :2], v[..., :11], v[0], v.double(), [1.0]):
            kw = dict(prior_mean=v, prior_std=v, init=v)
            kw[name] = bad
            with pytest.raises(ValueError, match=f"{name} must be a float32 tensor \\[1, 3, 12, 12\\]"):
                run(**kw)
    with pytest.raises(TypeError):
        U.XLFMDeconv(otf, img, 2, [12, 12], [24, 24], [12, 12, 3], None, 1, 10, 4500, "cuda:0", False, False, False, 0.999, False, None, 5, v)
    # valid arguments still need the device: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run(prior_mean=v, prior_std=v, init=v, accelerate=True, trace=True)
    o, tr = torch.ones(1, 3, 36, 36), torch.zeros(4, dtype=torch.float64)
    slab = torch.zeros(8, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.deconv_update_map(o, o.clone(), v, v.clone(), 12, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.deconv_update_accel_map(o, o.clone(), v, v.clone(), v.clone(), v.clone(), slab, 12, 12)
    with pytest.raises(ValueError, match="HIP device"):
        ops.deconv_penalty(torch.zeros(8, dtype=torch.float64), tr, 0)
    with pytest.raises(ValueError, match="penalty_slab"):
        ops.deconv_penalty(None, tr, 0)
