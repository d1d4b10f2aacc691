"""GPU: the trace post-processing against the numpy restatement tests/traces_ref.py, bit for bit: the sliding
quantile in both forms, the row select, the noise level, dF/F, the AR(1) deconvolution, and the planted scene through the public
functions."""
import numpy as np
import pytest
import torch

import traces_ref as R

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def strided(a, pad=7):
    """``a`` on the device as a view of a wider buffer: a row stride above T."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), -77.0, dtype=torch.float64, device="cuda")
    buf[:, :a.shape[1]] = dev(a)
    return buf[:, :a.shape[1]]


def same(t, want, what):
    got = host(t)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    bad = np.flatnonzero(got.view(np.uint64 if got.dtype == np.float64 else np.uint32).ravel() !=
                         want.view(np.uint64 if want.dtype == np.float64 else np.uint32).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}"


@pytest.fixture(scope="module")
def limits():
    from cwfa_amd import ops
    return ops.sliding_quantile_limits()


# ------------------------------------------------------------------------------------------------ sliding quantile
PS = (0, 8, 50, 99, 100)


@pytest.mark.parametrize("case", range(7))
def test_sliding_quantile_shapes(case, limits):
    from cwfa_amd import ops
    tile = limits[0]
    N, T = [(1, 1), (1, 2), (3, 7), (2, tile - 1), (2, tile), (2, tile + 1), (5, 2 * tile + 3)][case]
    rng = np.random.default_rng(case)
    x = np.where(rng.random((N, T)) < 0.5, np.round(rng.standard_normal((N, T)), 1), rng.standard_normal((N, T)))
    xd = dev(x)
    hs = sorted({h for h in (0, 1, 3, T - 2, T - 1, T + 5) if h >= 0} | ({tile + 44} if T > 2 * tile else set()))
    for h in hs:                                                                  # tile + 44: the halo spans more than one neighbouring segment
        for p in PS:
            want = R.sliding_quantile(x, h, p)
            lds, stream = ops.sliding_quantile(xd, h, p, form="lds"), ops.sliding_quantile(xd, h, p, form="stream")
            same(lds, want, f"lds {N}x{T} h {h} p {p}")
            same(stream, want, f"stream {N}x{T} h {h} p {p}")
            assert torch.equal(ops.sliding_quantile(xd, h, p), lds)


def test_sliding_quantile_lds_limit(limits):
    from cwfa_amd import ops
    from cwfa_amd._lib import CwfaHipError
    tile, most = limits
    T = 2 * most + tile + 9
    rng = np.random.default_rng(11)
    x = np.round(rng.standard_normal((1, T)), 2)
    xd = dev(x)
    at = [0, 1, most - 1, most, most + 1, T // 2, T - most - 2, T - most - 1, T - 2, T - 1]
    lds = ops.sliding_quantile(xd, most, 8, form="lds")
    same(lds[:, at], R.sliding_quantile(x, most, 8, at=at), "h = max_half_lds, lds")
    assert torch.equal(lds, ops.sliding_quantile(xd, most, 8, form="stream"))
    with pytest.raises(CwfaHipError, match="LDS form"):
        ops.sliding_quantile(xd, most + 1, 8, form="lds")
    auto = ops.sliding_quantile(xd, most + 1, 8)
    same(auto[:, at], R.sliding_quantile(x, most + 1, 8, at=at), "h = max_half_lds + 1, auto")
    assert torch.equal(auto, ops.sliding_quantile(xd, most + 1, 8, form="stream"))


def test_sliding_quantile_values():
    from cwfa_amd import ops
    x = R.value_rows(70)
    xd = strided(x)
    assert xd.stride(0) > 70
    for h in (0, 3, 9, 80):
        for p in (0, 8, 50, 100):
            want = R.sliding_quantile(x, h, p)
            for form in ("lds", "stream"):
                same(ops.sliding_quantile(xd, h, p, form=form), want, f"{form} h {h} p {p}")
    assert np.isnan(R.sliding_quantile(x, 3, 0)[9, :5]).all(), "the case holds an all-NaN window"


def test_sliding_quantile_empty_many_rows_and_repeatable():
    from cwfa_amd import ops
    for form in ("lds", "stream", "auto"):
        assert tuple(ops.sliding_quantile(torch.zeros(0, 5, dtype=torch.float64, device="cuda"), 2, 8, form=form).shape) == (0, 5)
    rng = np.random.default_rng(12)
    x = rng.standard_normal((70000, 3))
    xd = dev(x)
    want = R.sliding_quantile(x, 1, 50)
    for form in ("lds", "stream"):
        same(ops.sliding_quantile(xd, 1, 50, form=form), want, f"70000 rows, {form}")
    y = dev(np.round(rng.standard_normal((9, 700)), 1))
    for form in ("lds", "stream"):
        assert torch.equal(ops.sliding_quantile(y, 40, 8, form=form), ops.sliding_quantile(y, 40, 8, form=form))


# ------------------------------------------------------------------------------------------------ row select
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 1025])
def test_trace_select(T):
    from cwfa_amd import ops
    x = R.value_rows(T, seed=T)
    xd = strided(x)
    ranks = [0, (T - 1) // 2, T - 1]
    want = R.trace_select(x, ranks + [T // 3])
    same(ops.trace_select(xd, ranks + [T // 3]), want, f"T {T}, K = 4")
    for k, r in enumerate(ranks):
        same(ops.trace_select(xd, [r]), want[k:k + 1], f"T {T}, rank {r}")
    assert tuple(ops.trace_select(torch.zeros(0, T, dtype=torch.float64, device="cuda"), [0]).shape) == (1, 0)


# ------------------------------------------------------------------------------------------------ noise level and dF/F
def test_trace_noise():
    from cwfa_amd import CWFA
    rng = np.random.default_rng(13)
    x = 0.2 * rng.standard_normal((7, 301)) + 3.0
    x[2, 100] = np.nan
    x[3, ::3] = np.nan
    x[4] = 1.5
    same(CWFA.trace_noise(strided(x)), R.trace_noise(x), "trace_noise")
    assert np.isnan(R.trace_noise(x)[3]) and R.trace_noise(x)[4] == 0.0 and np.isfinite(R.trace_noise(x)[2])
    same(CWFA.trace_noise(dev(x[:, :2])), R.trace_noise(x[:, :2]), "T = 2")
    assert torch.isnan(CWFA.trace_noise(dev(x[:, :1]))).all()


def test_delta_f_over_f():
    from cwfa_amd import CWFA
    rng = np.random.default_rng(14)
    F = 2.0 + 0.3 * rng.standard_normal((6, 200))
    Fnp = 1.0 + 0.2 * rng.standard_normal((6, 200))
    Fnp[1] = np.nan                                                               # an empty shell: Fc = F
    F[2] -= 2.0                                                                   # a baseline at or below zero: NaN
    F[3, 50:80] = 0.0
    for fnp in (Fnp, None):
        for floor in (0.0, 1.2, 50.0):                                            # below, among and above the baselines
            got = CWFA.delta_f_over_f(strided(F), None if fnp is None else strided(fnp), alpha=0.7, half_window=12, percentile=8,
                                      floor=floor)
            want = R.delta_f_over_f(F, fnp, 0.7, 12, 8, floor)
            for g, w, name in zip(got, want, ("dff", "B", "D")):
                same(g, w, f"{name}, neuropil {fnp is not None}, floor {floor}")
            if fnp is None:
                assert got[2] is got[1]
    want = R.delta_f_over_f(F, Fnp, 0.7, 12, 8, 0.0)
    assert np.isnan(want[0][2]).any() and (want[2][2] <= 0).any() and R.same_bits(want[1][1], want[2][1])


# ------------------------------------------------------------------------------------------------ AR(1) deconvolution
def ar1_case(N, T, seed):
    rng = np.random.default_rng(seed)
    y = np.stack([R.ar1_response((rng.random(T) < 0.08) * (0.5 + rng.random(T)), 0.9) for _ in range(N)]) + 0.3 * rng.standard_normal((N, T))
    lam = np.array([0.0, 0.3, 5.0])[np.arange(N) % 3]
    t = np.arange(T, dtype=np.float64)
    rows = [10.0 * 0.8 ** t, 1.0 + t, np.concatenate([1.0 + t[:-1], [-1e6]])]   # one pool; T pools; the last sample merges many
    for n, r in enumerate(rows[:N]):
        y[n], lam[n] = r, 0.0
    if N >= 63:
        y[10, T // 2] = np.nan
        y[12, T - 1] = np.inf
        y[40, 0] = -np.inf
        lam[20], lam[33], lam[50] = np.nan, -0.5, np.inf
        y[N - 1], lam[N - 1] = 1.0 + t, 0.0                                       # the last row ends with T pools: the stacks' last slot is used
    return y, lam


@pytest.mark.parametrize("N,T", [(1, 1), (63, 2), (65, 3), (130, 64), (1, 65), (65, 65), (63, 600), (130, 600)])
def test_ar1_deconv(N, T):
    from cwfa_amd import ops
    y, lam = ar1_case(N, T, 100 * N + T)
    yd, ld = strided(y, 3), dev(lam)
    for gamma in ((0.0, 0.5, 0.95, 0.999) if N * T < 50000 else (0.95,)):
        want = R.ar1_deconv(y, gamma, lam)
        got = ops.ar1_deconv(yd, gamma, ld)
        for g, w, name in zip(got, want, ("c", "s", "pools")):
            same(g, w, f"{name}, N {N} T {T} gamma {gamma}")
        if gamma == 0.95 and T >= 64 and N >= 63:
            assert len(set(want[2][:64].tolist())) > 8, "rows of one wave differ in their pool counts"
            if N >= 3:
                assert want[2][0] == 1 and want[2][1] == T and want[2][2] < T - 20
        if N >= 63:
            assert want[2][[10, 12, 40, 20, 33, 50]].tolist() == [0] * 6 and (want[2][[9, 11, 13, 19, 21, 32, 34, 49, 51]] > 0).all()
            assert want[2][N - 1] == T
    again = ops.ar1_deconv(yd, 0.95, ld)
    once = ops.ar1_deconv(yd, 0.95, ld)
    assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
               for a, b in zip(again, once))


@pytest.mark.parametrize("N,T", [(1, 1), (3, 3), (65, 3), (5, 7)])
def test_ar1_deconv_stays_inside_its_workspace(N, T):
    """N T odd, every row rising (T pools each, so the last slot of every stack is written), the workspace exactly
    ``cwfa_ar1_deconv_workspace_bytes`` long inside a larger buffer: the doubles behind it keep their bits, and the last int32 of the
    lengths, which ends the 20 N T bytes, is written."""
    import ctypes as C
    from cwfa_amd import _lib, ops
    L = _lib.lib()
    nbytes = int(L.cwfa_ar1_deconv_workspace_bytes(N, T))
    assert nbytes % 8 == 0 and 20 * N * T <= nbytes < 20 * N * T + 8
    y = np.arange(1.0, N * T + 1.0).reshape(N, T)
    lam = np.zeros(N)
    guard = -77.25
    buf = torch.full((nbytes // 8 + 64,), guard, dtype=torch.float64, device="cuda")
    yd, ld, pw = dev(y), dev(lam), dev(R.powers(0.9, T))
    c, s = torch.empty(N, T, dtype=torch.float64, device="cuda"), torch.empty(N, T, dtype=torch.float64, device="cuda")
    pools = torch.empty(N, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(L.cwfa_ar1_deconv_f64(p(yd), N, T, T, 0.9, p(ld), p(pw), p(c), p(s), p(pools), p(buf), ops._stream()), "ar1_deconv")
    torch.cuda.synchronize()
    assert bool((buf[nbytes // 8:] == guard).all()), "a write behind the workspace"
    lengths = buf[:nbytes // 8].view(torch.int32)[4 * N * T:5 * N * T]
    assert lengths.tolist() == [1] * (N * T), "every slot of the length stack holds a pool of one sample"
    want = R.ar1_deconv(y, 0.9, lam)
    same(c, want[0], "c")
    same(pools, want[2], "pools")
    assert want[2].tolist() == [T] * N


def test_ar1_deconv_empty():
    from cwfa_amd import ops
    c, s, pools = ops.ar1_deconv(torch.zeros(0, 5, dtype=torch.float64, device="cuda"), 0.9, torch.zeros(0, dtype=torch.float64, device="cuda"))
    assert tuple(c.shape) == (0, 5) and tuple(s.shape) == (0, 5) and tuple(pools.shape) == (0,)


# ------------------------------------------------------------------------------------------------ the scene
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_scene_through_the_public_functions(seed):
    """The device's dF/F, noise level and deconvolution of the planted scene are the restatement's bits: what test_traces_cpu.py
    asserts of the restatement holds for the device's output."""
    from cwfa_amd import CWFA
    q = R.scene_pipeline(seed)
    dff, B, D = CWFA.delta_f_over_f(dev(q["F"]), half_window=75, percentile=10)
    same(dff, q["dff"], "dff")
    same(B, q["B"], "baseline")
    same(CWFA.trace_baseline(dev(q["F"]), 75, 10), q["B"], "trace_baseline")
    same(CWFA.trace_noise(dff), q["sigma"], "sigma")
    c, s, pools = CWFA.infer_spikes(dff, R.SCENE_GAMMA, lam_sigma=2.0)
    same(c, q["cd"], "c")
    same(s, q["sd"], "s")
    same(pools, q["pools"], "pools")
    lam = 2.0 * CWFA.trace_noise(dff)
    assert torch.equal(CWFA.infer_spikes(dff, R.SCENE_GAMMA, lam=lam)[0], c)
    same(CWFA.infer_spikes(dff, R.SCENE_GAMMA, lam=0.05)[0], R.ar1_deconv(q["dff"], R.SCENE_GAMMA, 0.05)[0], "a float lam")
