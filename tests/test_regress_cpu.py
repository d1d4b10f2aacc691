"""CPU: the streaming regression maps without a GPU -- the numpy restatement tests/regress_ref.py against
np.linalg.lstsq with an intercept column and the textbook formulae, its independence of the chunking, the refusals of the design, the
planted scene on which the GPU tests rely, the argument validation of the four entry points through the built library, and the
refusals the Python layer decides before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import neurons_ref as N
import regress_ref as R

EPS64 = 2.0 ** -52
T19 = 19
CHUNKS = [(1,) * 19, (8, 11), (19,), (1, 2, 16)]


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


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_is_least_squares_with_an_intercept():
    """T = 60 samples, K = 4 standard normal regressors, 5 x 6 x 7 voxels that follow them with random coefficients plus noise, float64
    both ways: np.linalg.lstsq on [1, r] per voxel and the textbook corr, t and R^2 from its residuals.

    The bound.  Every sum of the restatement is a recursive sum of T terms: its error is at most T eps64 times the sum of the absolute
    terms (Higham, Accuracy and Stability, eq. 4.4).  By Cauchy-Schwarz that sum is at most sqrt(s2 Srr_kk) for p_k, and s2, Srr_kk
    themselves for the squares; the centred quantities c_k, vx, G_kk that the maps are made of are smaller than these by the factors
    rho_x = max s2 / vx and rho_r = max Srr_kk / G_kk, which the test measures (the series is shifted by its first sample, the
    regressors are not shifted at all), so a centred quantity carries a relative error of at most (T + 2) eps64 sqrt(rho_x rho_r)
    (+ 2: the product and the centring).  beta = Ginv c solves a K x K system by Cholesky: the relative error of the solution is at
    most that of G and c times cond(G), plus K eps64 cond(G) of the factorisation and of the K-term products (Higham, theorem
    10.4, to first order), and lstsq's own backward error is of the same form.  corr, t and R^2 are quotients of such quantities
    without further cancellation (rss / vx is not small here: there is noise).  Both sides, each map relative to its largest
    magnitude:
        bound = 4 (T + K + 2) K cond(G) eps64 sqrt(rho_x rho_r)
    (4: the two sides, and numerator with denominator).  The draw has cond(G) < 100, asserted.  MEASURED (seed 5): cond(G) 2.36,
    rho_x 5.36, rho_r 1.03, bound 1.3e-12; worst difference over the bound: beta 0.0008, corr 0.0016, t 0.045, r2 0.0032
    (DESIGN.md section 34.4)."""
    rng = np.random.default_rng(5)
    T, K, shape = 60, 4, (5, 6, 7)
    rows = rng.standard_normal((T, K))
    coef = rng.standard_normal((K, *shape))
    x = (3.0 + np.tensordot(rows, coef, 1) + 0.5 * rng.standard_normal((T, *shape))).astype(np.float32)
    x0, s1, s2, p = R.accumulate(x, rows)
    sr, srr = R.rows_sums(rows)
    gdiag, ginv, status = R.design(sr, srr, T)
    assert status == (0, 0)
    # the maps in float64: the restatement's finish rounds to fp32 at the store, so the comparison reads them before that
    Nd = np.float64(T)
    vx = s2 - s1 * s1 / Nd
    c = np.stack([p[k] - s1 * sr[k] / Nd for k in range(K)])
    G = srr - np.outer(sr, sr) / Nd
    cond = float(np.linalg.cond(G))
    rho_x, rho_r = float((s2 / vx).max()), float((np.diag(srr) / np.diag(G)).max())
    bound = 4 * (T + K + 2) * K * cond * EPS64 * np.sqrt(rho_x * rho_r)
    assert cond < 100.0
    beta = np.stack([sum(ginv[k, l] * c[l] for l in range(K)) for k in range(K)])
    rss = np.maximum(vx - sum(c[k] * beta[k] for k in range(K)), 0.0)
    mine = {"beta": beta, "corr": np.stack([c[k] / np.sqrt(vx * gdiag[k]) for k in range(K)]),
            "t": np.stack([beta[k] / np.sqrt(rss / (T - K - 1) * ginv[k, k]) for k in range(K)]), "r2": 1.0 - rss / vx}
    # the textbook
    A = np.concatenate([np.ones((T, 1)), rows], 1)
    y = x.astype(np.float64).reshape(T, -1)
    sol = np.linalg.lstsq(A, y, rcond=None)[0]
    res = ((y - A @ sol) ** 2).sum(0)
    yc, rc = y - y.mean(0), rows - rows.mean(0)
    cov = np.linalg.inv(A.T @ A)
    want = {"beta": sol[1:].reshape(K, *shape),
            "corr": ((rc.T @ yc) / np.sqrt((rc ** 2).sum(0)[:, None] * (yc ** 2).sum(0)[None])).reshape(K, *shape),
            "t": (sol[1:] / np.sqrt(res[None] / (T - K - 1) * np.diag(cov)[1:, None])).reshape(K, *shape),
            "r2": (1.0 - res / (yc ** 2).sum(0)).reshape(shape)}
    worst = {}
    for name in want:
        worst[name] = float(np.abs(mine[name] - want[name]).max() / np.abs(want[name]).max()) / bound
    print(f"cond(G) {cond:.3g}, rho_x {rho_x:.3g}, rho_r {rho_r:.3g}, bound {bound:.3g}; worst difference / bound: "
          + ", ".join(f"{n} {v:.3g}" for n, v in worst.items()))
    assert max(worst.values()) <= 1.0
    # the fp32 maps of finish are these, rounded
    out = R.finish(s1, s2, p, sr, gdiag, ginv, T)
    for name in want:
        assert out[name].dtype == np.float32 and np.array_equal(out[name], mine[name].astype(np.float32))


def series(shape, K, T=T19):
    rng = np.random.default_rng(7)
    x = (100.0 + rng.standard_normal((T, *shape))).astype(np.float32)
    return x, rng.standard_normal((T, K))


@pytest.mark.parametrize("chunks", CHUNKS, ids=str)
def test_any_chunking_gives_the_same_bits(chunks):
    x, rows = series((3, 5, 4), 9)
    whole = R.accumulate(x, rows)
    state, t = None, 0
    for c in chunks:
        state = R.accumulate(x[t:t + c], rows[t:t + c], state)
        t += c
    assert t == T19
    for a, b in zip(state, whole):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for a, b in zip(R.rows_sums(rows, chunks), R.rows_sums(rows)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_the_design_flags_what_cannot_be_fitted():
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((T19, 3))
    assert R.design(*R.rows_sums(rows), T19)[2] == (0, 0)
    dup = rows.copy()
    dup[:, 2] = dup[:, 0]
    gdiag, ginv, status = R.design(*R.rows_sums(dup), T19)
    assert status == (R.COLLINEAR, 2) and not gdiag.any() and not ginv.any()
    comb = rows.copy()
    comb[:, 1] = 2.0 * comb[:, 0] - 0.5 * comb[:, 2]
    assert R.design(*R.rows_sums(comb), T19)[2] == (R.COLLINEAR, 2), "the last of a dependent set is the one reported"
    for value in (0.0, 1.0, 0.1, -2.5e3):
        const = rows.copy()
        const[:, 1] = value
        assert R.design(*R.rows_sums(const), T19)[2] == (R.COLLINEAR, 1), f"a regressor that is {value} throughout"
    for bad in (np.nan, np.inf, -np.inf):
        nan = rows.copy()
        nan[4, 1] = bad
        assert R.design(*R.rows_sums(nan), T19)[2] == (R.NONFINITE, 1)
    # near-collinear beyond rcond is refused, within it is fitted
    near = rows.copy()
    near[:, 2] = near[:, 0] + 1e-6 * near[:, 2]
    assert R.design(*R.rows_sums(near), T19)[2] == (R.COLLINEAR, 2) and R.design(*R.rows_sums(near), T19, rcond=1e-16)[2] == (0, 0)


def test_special_series_score_zero():
    x, rows = series((2, 3, 4), 2)
    y = x.copy()
    y[:, 0, 1, 1] = 3.25
    y[5, 1, 1, 2] = np.nan
    y[7, 1, 2, 0] = np.inf
    y[0, 0, 2, 3] = -np.inf
    clean, (code, _) = R.maps(x, rows)
    got, _ = R.maps(y, rows)
    planted = [(0, 1, 1), (1, 1, 2), (1, 2, 0), (0, 2, 3)]
    mask = np.zeros(x.shape[1:], dtype=bool)
    for v in planted:
        mask[v] = True
    assert code == 0
    for name in got:
        assert not np.isnan(got[name]).any() and not got[name][..., mask].any(), f"{name}: 0 where the series is degenerate"
        assert np.array_equal(got[name][..., ~mask].view(np.uint32), clean[name][..., ~mask].view(np.uint32)), "the others are untouched"
        assert clean[name][..., mask].all()


# ------------------------------------------------------------------------------------------------ what the GPU tests rely on
def test_the_planted_scene_separates_with_a_margin():
    """The thresholds of tests/test_gpu_regress.py, on the restatement alone: t of a planted centre is at least 4 times the
    threshold 10 and nothing away from the blobs of that regressor reaches half of it; the std map at threshold 3 finds all twelve
    blobs; the seed's correlation outside its blob stays below 0.25 (the GPU test allows 0.30).  MEASURED (seed 0): t >= 63.5 at the
    centres, <= 4.45 elsewhere; std >= 4.96 at the centres, <= 1.17 elsewhere; seed corr >= 0.967 inside, <= 0.249 outside."""
    x, rows, events, planted = R.scene(0)
    m, status = R.maps(x, rows)
    assert status == (0, 0)
    every = [c for k in R.CENTRES for c in R.CENTRES[k]]
    for k in range(3):
        t = m["t"][k]
        near = np.zeros(R.SHAPE, dtype=bool)
        for c in R.CENTRES[k]:
            near |= R.blob(c) > 1e-3
        lo, hi = min(float(t[c]) for c in R.CENTRES[k]), float(t[~near].max())
        print(f"regressor {k}: t at the centres >= {lo:.3g}, elsewhere <= {hi:.3g}")
        assert lo >= 40.0 and hi <= 5.0
        zyx = N.local_maxima(t, 10.0, R.DIST, R.MARGIN)[0]
        assert sorted(map(tuple, zyx.tolist())) == sorted(R.CENTRES[k])
    sd = x.astype(np.float64).std(0, ddof=1).astype(np.float32)
    near = np.zeros(R.SHAPE, dtype=bool)
    for c in every:
        near |= R.blob(c) > 1e-3
    print(f"std at the centres >= {min(float(sd[c]) for c in every):.3g}, elsewhere <= {float(sd[~near].max()):.3g}")
    assert min(float(sd[c]) for c in every) >= 4.5 and float(sd[~near].max()) <= 1.5
    assert sorted(map(tuple, N.local_maxima(sd, 3.0, R.DIST, R.MARGIN)[0].tolist())) == sorted(every)
    centre = R.CENTRES[None][0]
    trace, inside = R.seed_trace(x, centre)
    corr = R.maps(x, trace, want=("corr",))[0]["corr"][0]
    print(f"seed: corr >= {float(corr[inside].min()):.3g} on {int(inside.sum())} voxels inside, <= {float(corr[R.blob(centre) < 0.01].max()):.3g} outside")
    assert inside.sum() >= 5 and float(corr[inside].min()) > 0.93 and float(corr[R.blob(centre) < 0.01].max()) <= 0.25


def test_calcium_regressors_is_the_ar1_kernel():
    from cwfa_amd import CWFA
    events = R.scene(0)[2]
    got = CWFA.calcium_regressors(events, R.GAMMA, device="cpu")
    assert got.dtype == torch.float64 and tuple(got.shape) == events.shape
    assert np.array_equal(got.numpy().view(np.uint64), R.calcium(events, R.GAMMA).view(np.uint64))
    one = CWFA.calcium_regressors(torch.tensor([1.0, 0.0, 0.0, 2.0]), 0.5, device="cpu")
    assert one.tolist() == [[1.0], [0.5], [0.25], [2.125]]
    with pytest.raises(ValueError, match="gamma"):
        CWFA.calcium_regressors(events, 1.0, device="cpu")
    with pytest.raises(ValueError, match=r"\[T\] or \[T,K\]"):
        CWFA.calcium_regressors(np.zeros((2, 2, 2)), 0.5, device="cpu")


# ------------------------------------------------------------------------------------------------ the entry points' arguments
def test_activity_update_regress_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(8)]
    call = lambda a=q, T=1, K=2, m=8, ss=8, first=1: L.cwfa_activity_update_regress_f32(*a, T, K, m, ss, first, None)
    for k in range(8):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_activity_update_regress_f32: null" in L.cwfa_last_error()
    assert call(T=-1, first=0) == -2 and call(m=-8) == -2 and b"negative" in L.cwfa_last_error()
    for K in (0, 17, -1):
        assert call(K=K) == -2 and b"regressors" in L.cwfa_last_error()
    assert call(T=2, ss=7, first=0) == -1 and b"stride" in L.cwfa_last_error()
    assert call(T=0) == -2 and b"first chunk" in L.cwfa_last_error()
    assert call(first=2) == -1
    for k in (1, 3, 4, 7):
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert call(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    for K in (1, 8, 9, 16):
        assert call(T=0, first=0, K=K) == 0 and call(T=3, m=0, ss=0, K=K) == 0, "empty: no launch"


def test_regress_rows_and_design_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(4)]
    rows = lambda a=q, T=3, K=2, first=0: L.cwfa_regress_rows_f64(a[0], T, K, a[1], a[2], a[3], first, None)
    for k in range(4):
        args = list(q)
        args[k] = None
        assert rows(args) == -1 and b"cwfa_regress_rows_f64: null" in L.cwfa_last_error()
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert rows(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    assert rows(T=-1) == -2 and rows(K=0) == -2 and rows(K=17) == -2 and b"regressors" in L.cwfa_last_error()
    assert rows(first=2) == -1
    assert rows(T=0) == 0, "empty: no launch"
    d = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(6)]
    design = lambda a=d, N=5, K=2, rcond=1e-10: L.cwfa_regress_design_f64(a[0], a[1], a[2], N, K, rcond, a[3], a[4], a[5], None)
    for k in range(6):
        args = list(d)
        args[k] = None
        assert design(args) == -1 and b"cwfa_regress_design_f64: null" in L.cwfa_last_error()
        odd = list(d)
        odd[k] = ctypes.c_void_p(d[k].value + (4 if k < 5 else 2))
        assert design(odd) == -3 and b"aligned" in L.cwfa_last_error()
    assert design(K=0) == -2 and design(K=17) == -2 and design(N=0) == -2 and design(N=1 << 31) == -2
    assert design(rcond=-1.0) == -1 and design(rcond=1.0) == -1 and design(rcond=float("nan")) == -1


def test_regress_finish_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(10)]
    call = lambda a=q, N=9, K=2, m=8, want=15: L.cwfa_regress_finish_f32(*a[:6], N, K, m, want, *a[6:], None)
    for k in range(6):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_regress_finish_f32: null" in L.cwfa_last_error()
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert call(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    for k, bit in zip(range(6, 10), (1, 2, 4, 8)):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"requested output" in L.cwfa_last_error()
        assert call(args, m=0, want=15 - bit) == 0, "an output that is not requested may be null"
    assert call(want=0) == -1 and call(want=16) == -1
    assert call(K=0) == -2 and call(K=17) == -2 and call(N=0) == -2 and call(m=-1) == -2
    assert call(N=3, K=2) == -2 and b"degrees of freedom" in L.cwfa_last_error()
    assert call(N=3, K=2, want=11, m=0) == 0 and call(m=0) == 0, "empty: no launch; without t three samples are enough"


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_the_python_layer_refuses_before_any_device_work(built_lib):
    from cwfa_amd import CWFA, _lib, ops
    assert _lib.REGRESS_MAX_K == R.MAX_K and list(_lib.REGRESS_WANT) == ["corr", "beta", "t", "r2"]
    shape = (2, 3, 4)
    st = ops.regression_state(shape, "cpu", 3)
    assert st.p.shape == (3, *shape) and st.p.dtype == torch.float64 and st.sr.shape == (3,) and st.srr.shape == (3, 3)
    assert st.rows.dtype == torch.int64 and len(st.plain) == 5 and st.plain[1].dtype == torch.float64
    for k in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="regressors"):
            ops.regression_state(shape, "cpu", k)
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        ops.regression_state((3, 4), "cpu", 2)
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        CWFA.RegressionMap((3, 4), "cpu", 2)
    rm = CWFA.RegressionMap(shape, "cpu", 3)
    assert rm.count == 0 and rm.n_regressors == 3 and rm.state is rm.reg.plain
    x, rows = torch.zeros(2, *shape), torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="volumes of shape"):
        rm.update(torch.zeros(2, 2, 3, 5), rows)
    with pytest.raises(ValueError, match="volumes of shape"):
        rm.update(x[0], rows)
    with pytest.raises(ValueError, match="3 rows for 2 volumes"):
        rm.update(x, torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        rm.update(x, rows.float())
    with pytest.raises(ValueError, match="float64"):
        rm.update(x, torch.zeros(2, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rm.update(x, rows)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rm.update(x[0], rows[0])
    assert rm.count == 0
    with pytest.raises(ValueError, match="no volume"):
        rm.finish()
    with pytest.raises(ValueError, match="no volume"):
        rm.activity()
    rm.count = 4
    with pytest.raises(ValueError, match="degrees of freedom"):
        rm.finish()
    with pytest.raises(ValueError, match="degrees of freedom"):
        rm.finish(want=("t",))
    with pytest.raises(ValueError, match="subset"):
        rm.finish(want=("corr", "f"))
    with pytest.raises(ValueError, match="subset"):
        rm.finish(want=())
    with pytest.raises(ValueError, match="HIP device"):
        rm.finish(want=("corr", "beta", "r2"))
    with pytest.raises(ValueError, match="regressor is 0 .. 2"):
        CWFA.find_neurons(rm, kind="t")
    with pytest.raises(ValueError, match="regressor is 0 .. 2"):
        CWFA.find_neurons(rm, kind="beta", regressor=3)
    with pytest.raises(ValueError, match="for a RegressionMap"):
        CWFA.find_neurons(CWFA.ActivityMap(shape, "cpu"), regressor=0)
    with pytest.raises(ValueError, match="ActivityMap"):
        rm.activity("corr")
    with pytest.raises(ValueError, match="HIP device"):
        ops.regress_rows(rows, st, True)
    assert CWFA.find_neurons.__kwdefaults__ == {"regressor": None} and CWFA.find_neurons.__defaults__[-1] == "std"
    assert {"RegressionMap", "RegressionMaps", "calcium_regressors"} <= set(CWFA.__all__)
