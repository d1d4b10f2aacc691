"""The numpy restatement of the streaming regression maps, test infrastructure only: explicit float64 loops over
time and over the regressors, vectorised over voxels only, every operation in the order the kernels of regress_ops.hip perform it (no
matrix product, no library solve), so that the results are held to the bit.  Also the planted scene of the end-to-end tests."""
import numpy as np

MAX_K = 16
COLLINEAR, NONFINITE, COUNT = 1, 2, 3


def accumulate(x, rows, state=None):
    """(x0 fp32, s1, s2, p [K, ...]) of the series x [T, ...] (fp32) and its regressor rows [T, K] (float64): the sums over the samples
    after the first, in time order.  ``state``: what an earlier chunk returned, to which this chunk is added (every sample of it)."""
    x = np.asarray(x)
    rows = np.asarray(rows, dtype=np.float64)
    assert x.dtype == np.float32 and rows.shape[0] == x.shape[0]
    K = rows.shape[1]
    if state is None:
        x0, start = x[0].copy(), 1
        s1, s2, p = np.zeros(x0.shape), np.zeros(x0.shape), np.zeros((K, *x0.shape))
    else:
        x0, s1, s2, p = state
        p, start = p.copy(), 0
    b = x0.astype(np.float64)
    with np.errstate(all="ignore"):
        for t in range(start, x.shape[0]):
            d = x[t].astype(np.float64) - b
            s1 = s1 + d
            s2 = s2 + d * d
            for k in range(K):
                p[k] = p[k] + d * rows[t, k]
    return x0, s1, s2, p


def rows_sums(rows, chunks=None):
    """(Sr [K], Srr [K, K]) over all rows in time order; ``chunks`` (sizes) only shows that the cut does not matter."""
    rows = np.asarray(rows, dtype=np.float64)
    T, K = rows.shape
    sr, srr = np.zeros(K), np.zeros((K, K))
    t0 = 0
    with np.errstate(all="ignore"):
        for c in (chunks or (T,)):
            for t in range(t0, t0 + c):
                for k in range(K):
                    sr[k] = sr[k] + rows[t, k]
                    for l in range(K):
                        srr[k, l] = srr[k, l] + rows[t, k] * rows[t, l]
            t0 += c
    assert t0 == T
    return sr, srr


def design(sr, srr, N, rcond=1e-10):
    """(gdiag [K], ginv [K, K], (code, regressor)): G = Srr - Sr Sr' / N, its Cholesky factor row by row, the factor's inverse column
    by column and Ginv = Linv' Linv, as one thread of regress_design_kernel does it.  On a non-zero code gdiag and ginv are 0."""
    K = sr.shape[0]
    N = np.float64(N)
    gdiag, ginv = np.zeros(K), np.zeros((K, K))
    for whole_row in (False, True):
        for k in range(K):
            if not (np.isfinite(sr[k]) and np.isfinite(srr[k, k]) and (not whole_row or np.isfinite(srr[k]).all())):
                return gdiag, ginv, (NONFINITE, k)
    G, L, Li = np.zeros((K, K)), np.zeros((K, K)), np.zeros((K, K))
    for k in range(K):
        for l in range(k + 1):
            G[k, l] = srr[k, l] - sr[k] * sr[l] / N
    for j in range(K):
        s = G[j, j]
        for q in range(j):
            s = s - L[j, q] * L[j, q]
        if not (s > rcond * G[j, j]) or not (G[j, j] > rcond * srr[j, j]):
            return gdiag, ginv, (COLLINEAR, j)
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, K):
            u = G[i, j]
            for q in range(j):
                u = u - L[i, q] * L[j, q]
            L[i, j] = u / L[j, j]
    for c in range(K):
        Li[c, c] = 1.0 / L[c, c]
        for i in range(c + 1, K):
            u = np.float64(0.0)
            for q in range(c, i):
                u = u - L[i, q] * Li[q, c]
            Li[i, c] = u / L[i, i]
    for k in range(K):
        gdiag[k] = G[k, k]
        for l in range(K):
            u = np.float64(0.0)
            for q in range(max(k, l), K):
                u = u + Li[q, k] * Li[q, l]
            ginv[k, l] = u
    return gdiag, ginv, (0, 0)


def finish(s1, s2, p, sr, gdiag, ginv, N, want=("corr", "beta", "t", "r2")):
    """{name: fp32 map} for the names of ``want``: the per-voxel finish of regress_finish_kernel."""
    K = p.shape[0]
    Nd = np.float64(N)
    out = {}
    with np.errstate(all="ignore"):
        vx = s2 - s1 * s1 / Nd
        ok = (vx > 0.0) & np.isfinite(s1) & np.isfinite(s2)
        c = np.zeros_like(p)
        for k in range(K):
            ok = ok & np.isfinite(p[k])
            c[k] = p[k] - s1 * sr[k] / Nd
        beta = np.zeros_like(p)
        fit = np.zeros_like(s1)
        for k in range(K):
            u = np.zeros_like(s1)
            for l in range(K):
                u = u + ginv[k, l] * c[l]
            beta[k] = u
            fit = fit + c[k] * u
        res = vx - fit
        rss = np.where(res > 0.0, res, 0.0)
        f32 = lambda v, good: np.where(good, v, 0.0).astype(np.float32)
        if "corr" in want:
            out["corr"] = np.stack([f32(c[k] / np.sqrt(vx * gdiag[k]), ok) for k in range(K)])
        if "beta" in want:
            out["beta"] = np.stack([f32(beta[k], ok) for k in range(K)])
        if "t" in want:
            dof = np.float64(N - K - 1)
            assert dof >= 1
            s = rss / dof
            den = [np.sqrt(s * ginv[k, k]) for k in range(K)]
            out["t"] = np.stack([f32(beta[k] / den[k], ok & (den[k] != 0.0)) for k in range(K)])
        if "r2" in want:
            out["r2"] = f32(1.0 - rss / vx, ok)
    return out


def maps(x, rows, want=("corr", "beta", "t", "r2"), rcond=1e-10):
    """The whole path on a resident series: ({name: map}, (code, regressor))."""
    x0, s1, s2, p = accumulate(x, rows)
    sr, srr = rows_sums(rows)
    gdiag, ginv, status = design(sr, srr, x.shape[0], rcond)
    return finish(s1, s2, p, sr, gdiag, ginv, x.shape[0], want), status


def calcium(events, gamma):
    """c[t] = gamma c[t-1] + e[t] per column, float64."""
    e = np.asarray(events, dtype=np.float64)
    c, prev = np.empty_like(e), np.zeros(e.shape[1])
    for t in range(e.shape[0]):
        prev = gamma * prev + e[t]
        c[t] = prev
    return c


# ------------------------------------------------------------------------------------------------ the planted scene
SHAPE, T, GAMMA, SIGMA, AMP, BASE = (6, 36, 44), 200, 0.8, 1.0, 5.0, 100.0
R12, R3, MARGIN, DIST = 3, 1, (1, 3, 3), (1, 5, 5)
# blob centres (z, y, x), at least 8 apart in the plane; three per regressor, three unresponsive
CENTRES = {0: [(1, 6, 6), (3, 6, 18), (4, 6, 30)], 1: [(2, 17, 8), (1, 17, 22), (4, 17, 36)], 2: [(3, 28, 6), (2, 28, 20), (1, 28, 34)],
           None: [(4, 6, 40), (4, 28, 40), (4, 26, 28)]}


def blob(centre, shape=SHAPE, sz=0.7, sxy=1.2):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return np.exp(-0.5 * (((z - centre[0]) / sz) ** 2 + ((y - centre[1]) / sxy) ** 2 + ((x - centre[2]) / sxy) ** 2))


def scene(seed=0):
    """(stack fp32 [T, *SHAPE], regressors float64 [T, 3], events [T, 3], planted coefficients [3]): the regressors are sparse events
    through the calcium kernel; a responsive blob's peak follows its regressor with the coefficient AMP / std(regressor), an
    unresponsive blob a private event train with the same temporal variance; on a BASE background, plus white Gaussian noise of
    SIGMA."""
    rng = np.random.default_rng(100 + seed)
    events = (rng.random((T, 3)) < 0.08).astype(np.float64)
    R = calcium(events, GAMMA)
    planted = AMP / R.std(0)
    x = np.full((T, *SHAPE), BASE)
    for k in (0, 1, 2):
        for c in CENTRES[k]:
            x += planted[k] * R[:, k][:, None, None, None] * blob(c)[None]
    for c in CENTRES[None]:
        own = calcium((rng.random((T, 1)) < 0.08).astype(np.float64), GAMMA)[:, 0]
        x += AMP * (own / own.std())[:, None, None, None] * blob(c)[None]
    x += SIGMA * rng.standard_normal(x.shape)
    return x.astype(np.float32), R, events, planted


def seed_trace(x, centre, level=0.6):
    """(the mean trace of the voxels where the blob at ``centre`` is at least ``level``, float64 [T, 1]; that mask)."""
    inside = blob(centre) >= level
    return x[:, inside].astype(np.float64).mean(1)[:, None], inside
