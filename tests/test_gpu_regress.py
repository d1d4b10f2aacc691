"""GPU: the streaming regression maps.  The state of cwfa_activity_update_regress_f32 / cwfa_regress_rows_f64
against the numpy restatement tests/regress_ref.py and against an ActivityMap fed the same chunks, bit for bit, for the one-launch and
two-launch forms, every chunking of section 22 and the smallest shapes at which the kernel can go wrong; every finished map against
the restatement, bit for bit; special values; one volume larger than a pass of the grid against float64 torch operators on the
device; and planted scene -> calcium_regressors -> RegressionMap -> find_neurons(kind="t"), and a seed map."""
import functools

import numpy as np
import pytest
import torch

import regress_ref as R

pytestmark = pytest.mark.gpu

T = 19
SHAPES = [(1, 1, 1), (1, 1, 7), (2, 2, 2), (3, 5, 4), (2, 3, 8), (6, 36, 44), (7, 37, 45)]
KS = [1, 3, 8, 9, 16]
CHUNKS = [(1,) * 19, (0,) * 19, (8, 11), (19,), (1, 2, 16), "strided"]
NAMES = ("corr", "beta", "t", "r2")


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def stack(shape):
    """(host, device) [T, *shape]: a mean of 100, a spread of 1, and one constant voxel."""
    rng = np.random.default_rng(11)
    x = (100.0 + rng.standard_normal((T, *shape))).astype(np.float32)
    x[:, 0, 0, 0] = 3.25
    x.setflags(write=False)
    return x, torch.tensor(x).cuda()


@functools.lru_cache(maxsize=None)
def regressors(K):
    """(host, device) float64 [T, K]: standard normal around 0.5, so that neither the sums nor the cross terms vanish."""
    r = 0.5 + np.random.default_rng(12).standard_normal((T, K))
    r.setflags(write=False)
    return r, torch.tensor(r).cuda()


@functools.lru_cache(maxsize=None)
def reference(shape, K):
    x, r = stack(shape)[0], regressors(K)[0]
    x0, s1, s2, p = R.accumulate(x, r)
    sr, srr = R.rows_sums(r)
    gdiag, ginv, status = R.design(sr, srr, T)
    assert status == (0, 0)
    return x0, s1, s2, p, sr, srr, R.finish(s1, s2, p, sr, gdiag, ginv, T)


def feed(x, rows, chunks, m, with_rows=True):
    """The chunkings of section 22: sizes, 0 for one volume as [D,H,W] (with its row as [K]), or "strided": 8 + 11 of a view whose
    time stride exceeds a volume."""
    if chunks == "strided":
        n, vox = x.shape[0], x[0].numel()
        wide = torch.zeros(n, vox + 8, device="cuda")
        wide[:, :vox] = x.reshape(n, vox)
        view = wide.as_strided(tuple(x.shape), (vox + 8, x.shape[2] * x.shape[3], x.shape[3], 1))
        assert view.stride(0) == vox + 8 and torch.equal(view, x)
        x, chunks = view, (8, 11)
    t = 0
    for c in chunks:
        sl = t if c == 0 else slice(t, t + c)
        m.update(x[sl], rows[sl]) if with_rows else m.update(x[sl])
        t += max(c, 1)
    assert t == x.shape[0] and m.count == t
    return m


@functools.lru_cache(maxsize=None)
def plain_map(shape, chunks):
    from cwfa_amd.CWFA import ActivityMap
    return feed(stack(shape)[1], None, chunks, ActivityMap(shape, "cuda"), with_rows=False)


# ------------------------------------------------------------------------------------------------ the state and the maps
@pytest.mark.parametrize("chunks", CHUNKS, ids=str)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_state_and_maps_are_the_restatement_bit_for_bit(shape, K, chunks):
    from cwfa_amd.CWFA import RegressionMap
    x0, s1, s2, p, sr, srr, maps = reference(shape, K)
    rm = feed(stack(shape)[1], regressors(K)[1], chunks, RegressionMap(shape, "cuda", K))
    assert same_bits(rm.reg.p, p), "p differs from the restatement"
    assert same_bits(rm.reg.sr, sr) and same_bits(rm.reg.srr, srr) and int(rm.reg.rows.cpu()) == T, "Sr / Srr / the row count"
    assert same_bits(rm.state[0], x0) and same_bits(rm.state[1], s1) and same_bits(rm.state[2], s2), "x0 / s1 / s2 differ from the restatement"
    am = plain_map(shape, chunks)
    for a, b in zip(rm.state, am.state):
        assert same_bits(a, b), "the plain state differs from what an ActivityMap holds after the same chunks"
    got = rm.finish()
    for name in NAMES:
        g = getattr(got, name)
        worst = float(np.abs(g.cpu().numpy().astype(np.float64) - maps[name].astype(np.float64)).max())
        print(f"{shape} K={K} {chunks}: {name} differs from the restatement by at most {worst:.3g}; bitwise equal: {same_bits(g, maps[name])}")
        assert not bool(torch.isnan(g).any()) and same_bits(g, maps[name]), name
        assert not bool(g[..., 0, 0, 0].any()), "the constant voxel"
    assert rm.count == T and all(same_bits(a, b) for a, b in zip(rm.finish(), got)), "finish keeps the state"
    for kind in ("std", "snr"):
        assert all(same_bits(a, b) for a, b in zip(rm.activity(kind), am.finish(kind))), "activity() is ActivityMap.finish()"


def test_a_subset_of_the_maps():
    from cwfa_amd.CWFA import RegressionMap
    shape, K = (3, 5, 4), 3
    maps = reference(shape, K)[6]
    rm = feed(stack(shape)[1], regressors(K)[1], (8, 11), RegressionMap(shape, "cuda", K))
    for want in (("t",), ("r2", "corr"), "beta", ("corr", "beta", "r2")):
        got = rm.finish(want=want)
        for name in NAMES:
            if name in ((want,) if isinstance(want, str) else want):
                assert same_bits(getattr(got, name), maps[name])
            else:
                assert getattr(got, name) is None
    three = RegressionMap(shape, "cuda", 2).update(stack(shape)[1][:3], regressors(2)[1][:3])
    with pytest.raises(ValueError, match="degrees of freedom"):
        three.finish()
    ref = R.maps(stack(shape)[0][:3], regressors(2)[0][:3], want=("corr", "beta", "r2"))[0]
    got = three.finish(want=("corr", "beta", "r2"))
    assert all(same_bits(getattr(got, n), ref[n]) for n in ref) and got.t is None


def test_special_values():
    """A constant voxel, a NaN sample and an inf sample (also as the first sample) give 0 in every map; every other voxel keeps its
    bits.  Collinear, constant and non-finite regressors raise at finish."""
    from cwfa_amd.CWFA import RegressionMap
    shape, K = (2, 3, 8), 3
    x, r = stack(shape)[0], regressors(K)
    y = x.copy()
    y[5, 1, 1, 2] = np.nan
    y[7, 1, 2, 0] = np.inf
    y[0, 0, 2, 3] = -np.inf
    planted = np.zeros(shape, dtype=bool)
    for v in ((0, 0, 0), (1, 1, 2), (1, 2, 0), (0, 2, 3)):
        planted[v] = True
    run = lambda a, rows, k=K: feed(torch.tensor(a).cuda(), rows, (1, 2, 16), RegressionMap(shape, "cuda", k))
    clean, got, ref = run(x, r[1]).finish(), run(y, r[1]).finish(), R.maps(y, r[0])[0]
    for name in NAMES:
        g, c = getattr(got, name).cpu().numpy(), getattr(clean, name).cpu().numpy()
        assert same_bits(g, ref[name]) and not np.isnan(g).any()
        assert not g[..., planted].any(), f"{name}: 0 where the series is degenerate"
        assert np.array_equal(bits(g)[..., ~planted], bits(c)[..., ~planted]), "the neighbours are untouched"
        assert c[..., ~planted].all()
    dup = r[1].clone()
    dup[:, 2] = dup[:, 0]
    with pytest.raises(ValueError, match="collinear or constant regressor 2"):
        run(x, dup).finish()
    const = r[1].clone()
    const[:, 1] = 0.1
    with pytest.raises(ValueError, match="collinear or constant regressor 1"):
        run(x, const).finish(want=("corr",))
    nan = r[1].clone()
    nan[4, 1] = float("nan")
    with pytest.raises(ValueError, match="regressor 1 .non-finite"):
        run(x, nan).finish()
    near = r[1].clone()
    near[:, 2] = near[:, 0] + 1e-6 * near[:, 2]
    m = run(x, near)
    with pytest.raises(ValueError, match="regressor 2"):
        m.finish()
    ref = R.maps(x, near.cpu().numpy(), rcond=1e-16)
    assert ref[1] == (0, 0) and all(same_bits(getattr(m.finish(rcond=1e-16), n), ref[0][n]) for n in NAMES)


# ------------------------------------------------------------------------------------------------ more voxels than one pass of the grid
def test_grid_stride_takes_two_steps():
    """33 x 512 x 512 voxels: more than the 8192 blocks x 256 threads x 4 voxels of one pass of the update kernel's grid.  T = 4 as
    1 + 3, K = 2, against sequential float64 torch operators on the device in the kernel's order."""
    from cwfa_amd.CWFA import RegressionMap
    shape = (33, 512, 512)
    assert shape[0] * shape[1] * shape[2] > 8192 * 256 * 4
    g = torch.Generator(device="cuda").manual_seed(2)
    x = 10.0 + torch.randn(4, *shape, device="cuda", generator=g)
    rows = regressors(2)[1][:4].contiguous()
    rm = RegressionMap(shape, "cuda", 2).update(x[:1], rows[:1]).update(x[1:], rows[1:])
    host = rows.cpu().tolist()
    x0 = x[0].double()
    s1, s2 = torch.zeros_like(x0), torch.zeros_like(x0)
    p = torch.zeros(2, *shape, dtype=torch.float64, device="cuda")
    for t in (1, 2, 3):
        d = x[t].double().sub(x0)
        s1 = s1.add(d)
        s2 = s2.add(d.mul(d))
        for k in range(2):
            p[k] = p[k].add(d.mul(host[t][k]))
    as_int = lambda t: t.view(torch.int64)
    assert torch.equal(as_int(rm.reg.p), as_int(p)), "p"
    assert torch.equal(as_int(rm.state[1]), as_int(s1)) and torch.equal(as_int(rm.state[2]), as_int(s2)) and torch.equal(rm.state[0], x[0])
    assert torch.equal(rm.state[3], x.amax(0)) and torch.equal(rm.state[4], x.amin(0))
    r2 = rm.finish(want=("r2",)).r2
    assert bool(((r2 >= 0.0) & (r2 <= 1.0)).all()) and float(r2.max()) > 0.0, "the finish kernel's grid covers the volume too"
    del x, p, rm
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def planted_scene():
    x, rows, events, planted = R.scene(0)
    return x, rows, events, planted, torch.tensor(x).cuda()


def test_the_planted_scene():
    """Every planted coefficient comes back within 5 sigma sqrt(Ginv_kk / n_eff), and find_neurons on the t-map of regressor k
    returns exactly the blobs planted on it, where the std map of the same state returns the unresponsive blobs as well.

    The bound: the least-squares estimate is beta + Ginv Rc' e with Rc the centred regressors and G = Rc' Rc (sums, not means), so
    under white noise e of variance sigma^2 it has covariance sigma^2 Ginv: a standard deviation of sigma sqrt(Ginv_kk) per voxel.
    The test reads one voxel, the blob's centre, where the blob's weight is 1: n_eff = 1.  What else enters is far below that
    0.07 / std(regressor): the fp32 rounding of the samples (2^-18 at 100), the tails of the other blobs (< 1e-9 at 8 voxels).  Five
    standard deviations: 6e-7 per coefficient."""
    from cwfa_amd import CWFA
    x, rows, events, planted, xd = planted_scene()
    rd = CWFA.calcium_regressors(events, R.GAMMA)
    assert rd.is_cuda and same_bits(rd, rows), "calcium_regressors is the restatement's AR(1) kernel"
    rm = CWFA.RegressionMap(R.SHAPE, "cuda", 3)
    for t in range(0, R.T, 16):
        rm.update(xd[t:t + 16], rd[t:t + 16])
    got = rm.finish()
    ref, status = R.maps(x, rows)
    assert status == (0, 0) and all(same_bits(getattr(got, n), ref[n]) for n in NAMES), "the maps are the restatement's"
    ginv = R.design(*R.rows_sums(rows), R.T)[1]
    beta = got.beta.cpu().numpy()
    for k in range(3):
        for c in R.CENTRES[k]:
            err, lim = abs(float(beta[k][c]) - planted[k]), 5.0 * R.SIGMA * np.sqrt(ginv[k, k] / 1.0)
            print(f"regressor {k} at {c}: beta {float(beta[k][c]):.4f}, planted {planted[k]:.4f}, |error| {err:.3g} <= {lim:.3g}")
            assert err <= lim
    shift = R.SHAPE[0] // 2 - 13
    find = lambda **kw: sorted((z + shift, y, xx) for xx, y, z in CWFA.find_neurons(rm, r12=R.R12, r3=R.R3, margin=R.MARGIN, dist=R.DIST, **kw)[0])
    for k in range(3):
        assert find(kind="t", regressor=k, thr=10.0) == sorted(R.CENTRES[k]), f"the blobs planted on regressor {k}, nothing else"
    every = sorted(c for k in R.CENTRES for c in R.CENTRES[k])
    assert find(thr=3.0) == every and find(kind="std", thr=3.0) == every, "the std map of the same state takes every blob for a neuron"
    coords, scores = CWFA.find_neurons(rm.activity("std")[0], r12=R.R12, r3=R.R3, margin=R.MARGIN, dist=R.DIST, thr=3.0)
    assert len(coords) == 12
    # corr and beta maps of a regressor find the same blobs
    assert find(kind="corr", regressor=1, thr=0.5) == sorted(R.CENTRES[1]) and find(kind="beta", regressor=2, thr=0.5 * planted[2]) == sorted(R.CENTRES[2])


def test_a_seed_map():
    """An unresponsive blob's own mean trace as the single regressor: corr is above 0.9 inside the blob (where the blob's weight is
    at least 0.6: a signal of variance >= 9 on noise of variance 1 gives 0.95), and outside it (weight below 0.01) below 0.30: the
    restatement's largest value there on this scene, 0.249 (tests/test_regress_cpu.py), plus a margin of 0.05."""
    from cwfa_amd import CWFA
    x, rows, events, planted, xd = planted_scene()
    centre = R.CENTRES[None][0]
    trace, inside = R.seed_trace(x, centre)
    rm = CWFA.RegressionMap(R.SHAPE, "cuda", 1)
    td = torch.tensor(trace).cuda()
    for t in range(0, R.T, 16):
        rm.update(xd[t:t + 16], td[t:t + 16])
    corr = rm.finish(want=("corr",)).corr[0].cpu().numpy()
    assert same_bits(corr, R.maps(x, trace, want=("corr",))[0]["corr"][0])
    outside = R.blob(centre) < 0.01
    print(f"seed map: corr >= {float(corr[inside].min()):.3f} inside, <= {float(corr[outside].max()):.3f} outside")
    assert float(corr[inside].min()) > 0.9 and float(corr[outside].max()) < 0.30
    found = CWFA.find_neurons(rm, r12=R.R12, r3=R.R3, margin=R.MARGIN, dist=R.DIST, kind="corr", regressor=0, thr=0.5)[0]
    assert [(z + R.SHAPE[0] // 2 - 13, y, xx) for xx, y, z in found] == [centre]
