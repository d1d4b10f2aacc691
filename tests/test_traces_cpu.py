"""CPU: the trace post-processing without a GPU -- the numpy restatement tests/traces_ref.py against brute
force, against scipy's NNLS and against the properties of the AR(1) solution; the purpose of the feature on the planted scene; the
argument validation of the new entry points through the built library; and the refusals the Python layer decides before any device
work."""
import ctypes

import numpy as np
import pytest
import torch

import traces_ref as R


@pytest.fixture(scope="module")
def built_lib():
    from cwfa_amd import _lib, build
    build.build_all()
    return _lib.lib()


@pytest.fixture(scope="module")
def ptr():
    buf = ctypes.create_string_buffer(16384)
    base = ctypes.addressof(buf)
    return ctypes.c_void_p((base + 15) & ~15)


# ------------------------------------------------------------------------------------------------ the restatement: quantiles
def test_sliding_quantile_against_sorted_windows():
    rng = np.random.default_rng(0)
    x = np.round(rng.standard_normal((3, 41)), 1)                                 # ties
    for h, p in ((0, 50), (1, 8), (3, 50), (7, 99), (20, 10), (39, 30)):
        got = R.sliding_quantile(x, h, p)
        for n in range(3):
            for t in range(41):
                w = sorted(x[n, max(0, t - h):min(40, t + h) + 1].tolist())
                assert got[n, t] == w[(p * (len(w) - 1)) // 100], (h, p, n, t)


def test_sliding_quantile_extremes_and_global():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 30))
    for h in (0, 2, 5):
        lo = np.array([[x[n, max(0, t - h):t + h + 1].min() for t in range(30)] for n in range(2)])
        hi = np.array([[x[n, max(0, t - h):t + h + 1].max() for t in range(30)] for n in range(2)])
        assert np.array_equal(R.sliding_quantile(x, h, 0), lo) and np.array_equal(R.sliding_quantile(x, h, 100), hi)
    for h in (29, 30, 1000):
        for p in (0, 8, 50, 100):
            want = np.sort(x, axis=1)[:, (p * 29) // 100]
            assert np.array_equal(R.sliding_quantile(x, h, p), np.repeat(want[:, None], 30, axis=1))


def test_the_order_of_special_values():
    neg_nan = np.array([0xfff8000000000123], dtype=np.uint64).view(np.float64)[0]
    tiny = np.array([0x3ff0000000000000, 0x3ff0000000000001], dtype=np.uint64).view(np.float64)
    s = R.ordered([np.inf, neg_nan, -0.0, tiny[1], 0.0, np.nan, tiny[0], -np.inf, -5e-324])
    assert R.bits(s).tolist() == [0xfff0000000000000, 0x8000000000000001, 0, 0, 0x3ff0000000000000, 0x3ff0000000000001, 0x7ff0000000000000,
                                  0x7ff8000000000000, 0x7ff8000000000000]
    assert R.same_bits(R.trace_select(np.array([[neg_nan, 1.0, -0.0]]), [0, 1, 2]), np.array([[0.0], [1.0], [R.QNAN]]))


# ------------------------------------------------------------------------------------------------ the restatement: deconvolution
GAMMAS, LAMS = (0.0, 0.5, 0.9, 0.95, 0.99), (0.0, 0.1, 0.5, 2.0)


def test_deconvolution_against_nnls():
    """K s ~ y - lam (1 - gamma, .., 1 - gamma, 1) with K[i, j] = gamma^(i - j): sum s_t = sum_t c_t (1 - gamma) + gamma c_{T-1}, so the
    L1 term is linear in c and folds into the data.  200 cases, T 1 .. 69; the bound is the 1e-9 of section 28.4 (NNLS has a tolerance
    of its own)."""
    nnls = pytest.importorskip("scipy.optimize", reason="scipy is needed for the NNLS cross-check").nnls
    rng = np.random.default_rng(5)
    worst = 0.0
    for case in range(200):
        T = int(rng.integers(1, 70))
        g, lam = GAMMAS[case % 5], LAMS[(case // 5) % 4]
        y = R.ar1_response((rng.random(T) < 0.1) * (0.5 + rng.random(T)), 0.9) + 0.3 * rng.standard_normal(T)
        c, s, _ = R.ar1_row(y, g, lam)
        i = np.arange(T)
        K = np.tril(np.float64(g) ** np.maximum(i[:, None] - i[None, :], 0))
        mu = np.full(T, lam * (1.0 - g))
        mu[-1] = lam
        sol = nnls(K, y - mu, maxiter=50 * T + 100)[0]
        worst = max(worst, float(np.abs(K @ sol - c).max()))
    print(f"largest |c - K nnls|: {worst:.2e}")
    assert worst <= 1e-9


def test_deconvolution_properties():
    rng = np.random.default_rng(6)
    for case in range(60):
        T = int(rng.integers(2, 120))
        g, lam = GAMMAS[case % 5], LAMS[(case // 5) % 4]
        y = R.ar1_response((rng.random(T) < 0.1) * (0.5 + rng.random(T)), 0.9) + 0.3 * rng.standard_normal(T)
        c, s, pools = R.ar1_row(y, g, lam)
        assert (s >= 0.0).all() and np.count_nonzero(s) <= pools <= T
        resid = c[1:] - np.float64(g) * c[:-1] - s[1:]
        assert np.abs(resid).max() <= 4 * np.finfo(np.float64).eps * max(1.0, np.abs(c).max()), (case, np.abs(resid).max())
        assert c[0] == s[0]
        if g == 0.0:
            mu = np.full(T, lam)
            assert np.array_equal(c, np.maximum(y - mu, 0.0)) and np.array_equal(s, c)


def test_deconvolution_returns_an_exact_response_at_lambda_zero():
    rng = np.random.default_rng(7)
    s0 = (rng.random(200) < 0.05) * (0.5 + rng.random(200))
    s0[0] = 1.0
    for g in (0.5, 0.9, 0.95):
        y = R.ar1_response(s0, g)
        c, s, pools = R.ar1_row(y, g, 0.0)
        assert np.abs(c - y).max() <= 1e-13 and np.abs(s - s0).max() <= 1e-13, g


def test_deconvolution_edges():
    assert [a.tolist() for a in R.ar1_row([2.0], 0.9, 0.5)[:2]] == [[1.5], [1.5]] and R.ar1_row([2.0], 0.9, 0.5)[2] == 1
    assert R.ar1_row([-2.0], 0.9, 0.5)[0].tolist() == [0.0]
    dec = R.ar1_row(10.0 * 0.8 ** np.arange(50), 0.95, 0.0)                      # falls faster than gamma^t: every sample merges
    inc = R.ar1_row(np.arange(1.0, 51.0), 0.95, 0.0)
    assert dec[2] == 1 and inc[2] == 50 and np.count_nonzero(dec[1]) == 1
    back = R.ar1_row(np.concatenate([np.arange(1.0, 40.0), [-1e6]]), 0.95, 0.0)
    assert back[2] < 10, "the last sample pulls the pools before it into one"
    for bad_y, lam in (([1.0, np.nan, 2.0], 0.1), ([1.0, np.inf, 2.0], 0.1), ([1.0, 2.0, 3.0], np.nan), ([1.0, 2.0, 3.0], -0.1),
                       ([1.0, 2.0, 3.0], np.inf)):
        c, s, pools = R.ar1_row(bad_y, 0.9, lam)
        assert pools == 0 and R.bits(c).tolist() == [0x7ff8000000000000] * 3 and R.same_bits(c, s)
    c, s, pools = R.ar1_deconv(np.array([[1.0, 2.0, 3.0], [1.0, np.nan, 3.0], [1.0, 2.0, 3.0]]), 0.9, [0.1, 0.1, 0.1])
    assert pools.tolist() == [3, 0, 3] and R.same_bits(c[0], c[2]) and np.isnan(c[1]).all()


def test_noise_level_on_white_noise():
    rng = np.random.default_rng(8)
    x = 0.37 * rng.standard_normal((6, 20000)) + 5.0
    sigma = R.trace_noise(x)
    print("sigma / 0.37:", (sigma / 0.37).round(4).tolist())
    assert np.abs(sigma / 0.37 - 1.0).max() < 0.03                               # the MAD of 19 999 differences: about 1 % (1 sigma)
    assert np.isnan(R.trace_noise(np.ones((2, 1)))).all() and R.trace_noise(np.ones((2, 2))).tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ what the feature is for
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_dff_and_the_denoised_trace_follow_the_planted_calcium(seed):
    q = R.scene_pipeline(seed)
    raw, dff, den = R.corr_rows(q["F"], q["c"]), R.corr_rows(q["dff"], q["c"]), R.corr_rows(q["cd"], q["c"])
    planted = np.count_nonzero(q["s"], axis=1)
    print(f"seed {seed}: corr raw {raw.round(3).tolist()}, dff {dff.round(3).tolist()}, denoised {den.round(3).tolist()}; "
          f"sigma / planted {(q['sigma'] * q['B'].mean(axis=1) / R.SCENE_NOISE).round(2).tolist()}; non-zero s "
          f"{np.count_nonzero(q['sd'], axis=1).tolist()} beside {planted.tolist()} planted spikes")
    assert (dff > raw).all()
    assert np.median(den) >= np.median(dff)
    assert (q["sd"] >= 0.0).all()


# ------------------------------------------------------------------------------------------------ the entry points' arguments
def test_sliding_quantile_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 4096 * k) for k in range(2)]
    tile, most = ctypes.c_int(0), ctypes.c_int(0)
    assert L.cwfa_sliding_quantile_limits(ctypes.byref(tile), ctypes.byref(most)) == 0 and tile.value >= 64 and most.value >= tile.value
    assert L.cwfa_sliding_quantile_limits(None, ctypes.byref(most)) == -1

    def call(x=q[0], N=1, T=8, stride=8, h=2, p=8, out=q[1], form=0):
        return L.cwfa_sliding_quantile_f64(x, N, T, stride, h, p, out, form, None)
    assert call(x=None) == -1 and b"cwfa_sliding_quantile_f64: null" in L.cwfa_last_error() and call(out=None) == -1
    assert call(N=-1) == -2 and call(T=0) == -2 and call(stride=7) == -1 and b"stride" in L.cwfa_last_error()
    assert call(T=1 << 30, stride=1 << 30) == -2 and b"2^30" in L.cwfa_last_error()
    assert call(p=-1) == -1 and call(p=101) == -1 and b"percentile" in L.cwfa_last_error()
    assert call(h=-1) == -1 and b"half window" in L.cwfa_last_error()
    assert call(form=3) == -1 and call(form=-1) == -1
    assert call(h=most.value + 1, form=1) == -2 and b"LDS form" in L.cwfa_last_error()
    assert call(x=ctypes.c_void_p(q[0].value + 4)) == -3 and call(out=ctypes.c_void_p(q[1].value + 4)) == -3
    assert call(N=0) == 0 and call(N=0, x=None, out=None) == 0 and call(N=0, h=most.value, form=1) == 0, "empty: no launch"


def test_trace_select_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 4096 * k) for k in range(2)]

    def call(x=q[0], N=1, T=8, stride=8, ranks=(0, 7), out=q[1], K=None):
        r = None if ranks is None else (ctypes.c_int * max(len(ranks), 1))(*ranks)
        return L.cwfa_trace_select_f64(x, N, T, stride, r, len(ranks or ()) if K is None else K, out, None)
    assert call(x=None) == -1 and b"cwfa_trace_select_f64: null" in L.cwfa_last_error() and call(out=None) == -1 and call(ranks=None, K=1) == -1
    assert call(N=-1) == -2 and call(T=0) == -2 and call(stride=7) == -1
    assert call(ranks=(), K=0) == -1 and call(ranks=(0,) * 5) == -1 and b"1 .. 4" in L.cwfa_last_error()
    assert call(ranks=(8,)) == -1 and call(ranks=(0, -1)) == -1 and b"rank" in L.cwfa_last_error()
    assert call(x=ctypes.c_void_p(q[0].value + 4)) == -3
    assert call(N=0) == 0 and call(N=0, x=None, out=None) == 0, "empty: no launch"


def test_ar1_deconv_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 2048 * k) for k in range(7)]                 # y, lam, pw, c, s, pools, ws

    def call(a=q, N=1, T=8, stride=8, gamma=0.9):
        return L.cwfa_ar1_deconv_f64(a[0], N, T, stride, gamma, *a[1:], None)
    for k in range(7):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_ar1_deconv_f64: null" in L.cwfa_last_error()
    assert call(N=-1) == -2 and call(T=0) == -2 and call(stride=7) == -1 and b"stride" in L.cwfa_last_error()
    for g in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert call(gamma=g) == -1 and b"gamma" in L.cwfa_last_error()
    for k in (0, 1, 2, 3, 4, 6):
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert call(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    assert call(N=0) == 0 and call([None, None, q[2], None, None, None, None], N=0) == 0, "empty: no launch"
    assert L.cwfa_ar1_deconv_workspace_bytes(3, 7) == 20 * 21 + 4 and L.cwfa_ar1_deconv_workspace_bytes(0, 7) == 0
    assert L.cwfa_ar1_deconv_workspace_bytes(1, 1) == 24, "the int32 lengths end a whole number of doubles"
    assert L.cwfa_ar1_deconv_workspace_bytes(4096, 10000) == 20 * 4096 * 10000
    assert L.cwfa_ar1_deconv_workspace_bytes(-1, 7) == -1 and L.cwfa_ar1_deconv_workspace_bytes(1, 0) == -1


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_the_python_layer_refuses_before_any_device_work(built_lib):
    from cwfa_amd import CWFA, ops
    assert {"trace_baseline", "delta_f_over_f", "trace_noise", "infer_spikes"} <= set(CWFA.__all__)
    tile, most = ops.sliding_quantile_limits()
    assert tile >= 64 and most >= tile
    x = torch.zeros(2, 9, dtype=torch.float64)
    calls = {"trace_baseline": lambda t: CWFA.trace_baseline(t, 3), "delta_f_over_f": lambda t: CWFA.delta_f_over_f(t, half_window=3),
             "trace_noise": CWFA.trace_noise, "infer_spikes": lambda t: CWFA.infer_spikes(t, 0.9, lam=0.1),
             "sliding_quantile": lambda t: ops.sliding_quantile(t, 3, 8), "trace_select": lambda t: ops.trace_select(t, [0]),
             "ar1_deconv": lambda t: ops.ar1_deconv(t, 0.9, torch.zeros(2, dtype=torch.float64))}
    for name, f in calls.items():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x)
        with pytest.raises(TypeError, match="float64"):
            f(x.float())
        with pytest.raises(ValueError, match=r"\[N, T\]"):
            f(x[0])
        with pytest.raises(ValueError, match=r"\[N, T\]"):
            f(x[:, :0])
        with pytest.raises(TypeError, match="torch.Tensor"):
            f(np.zeros((2, 9)))
    for bad in ({"half_window": -1}, {"half_window": 2.5}, {"half_window": 3, "percentile": 101}, {"half_window": 3, "percentile": -1},
                {"half_window": 3, "percentile": 8.5}):
        with pytest.raises(ValueError, match="half_window|percentile"):
            CWFA.trace_baseline(x, **bad)
        with pytest.raises(ValueError, match="half_window|percentile"):
            CWFA.delta_f_over_f(x, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # numpy integers are integers: the window is accepted
        CWFA.trace_baseline(x, np.int64(3), np.int32(8))
    with pytest.raises(ValueError, match="half_window"):
        CWFA.trace_baseline(x, True)
    with pytest.raises(ValueError, match="floor"):
        CWFA.delta_f_over_f(x, half_window=3, floor=-1.0)
    with pytest.raises(ValueError, match="floor"):
        CWFA.delta_f_over_f(x, half_window=3, floor=float("nan"))
    with pytest.raises(ValueError, match="form"):
        ops.sliding_quantile(x, 3, 8, form="fast")
    for ranks in ([], [0] * 5):
        with pytest.raises(ValueError, match="1 to 4 ranks"):
            ops.trace_select(x, ranks)
    with pytest.raises(ValueError, match="exactly one"):
        CWFA.infer_spikes(x, 0.9)
    with pytest.raises(ValueError, match="exactly one"):
        CWFA.infer_spikes(x, 0.9, lam=0.1, lam_sigma=2.0)
    for g in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            CWFA.infer_spikes(x, g, lam=0.1)
        with pytest.raises(ValueError, match="gamma"):
            ops.ar1_deconv(x, g, None)
