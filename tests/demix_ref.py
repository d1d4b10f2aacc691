"""The numpy restatement of the demixing of overlapping footprints and the scene its tests use.  No test functions
here; tests/test_demix_cpu.py and tests/test_gpu_demix.py import it.

    pairs    every (n, m), n <= m, whose boxes share a voxel, and every (n, n); ascending in (n, m)
    G_nm     = sum over the intersection of boxes n and m of w_n(v) w_m(v)              (math.fsum of the exact float64 products)
    M_nm     = (G_nm wsum_m) / (G_mm wsum_n) for m != n; 0.0 where G_nm == 0, where G_mm, wsum_n or their product is not > 0 and
               where either footprint is empty (sizes == 0)                             (three float64 operations, each rounded)
    solve    per time step, from f = F (NaN in the rows of empty footprints): a sweep visits n = 0 .. N-1; acc = 0.0; over the row's
             entries by ascending m, acc = acc + M_nm f_m where M_nm != 0.0; new = F_n - acc; nonneg: new < 0 becomes 0.0;
             a NaN becomes the NaN 0x7ff8000000000000; f_n = new.  The step ends after the first sweep in which every |new - old| <= tol (NaN is not; the rows of empty
             footprints do not count), or after n_sweeps.

The sweep's loops over n and over a row's entries are explicit; the time steps are the elements of numpy vectors, on which every
operation is elementwise: the bits per time step are those of a scalar loop."""
import functools
import math

import numpy as np

import footprints_ref as FR


# ------------------------------------------------------------------------------------------------ pairs and structure
def intersection(a, b):
    """The box [z0, z1, y0, y1, x0, x1] two boxes share, or None."""
    out = []
    for k in range(3):
        lo, hi = max(int(a[2 * k]), int(b[2 * k])), min(int(a[2 * k + 1]), int(b[2 * k + 1]))
        if hi <= lo:
            return None
        out += [lo, hi]
    return out


def pairs_of(boxes):
    """int32 [P,2] by the O(N^2) definition."""
    N = len(boxes)
    return np.array([(n, m) for n in range(N) for m in range(n, N) if n == m or intersection(boxes[n], boxes[m]) is not None],
                    dtype=np.int32).reshape(-1, 2)


def structure(pairs, N):
    """(rowptr int32 [N+1], col int32 [E]): (n, m) and (m, n) for every pair n < m, columns ascending within a row."""
    rows = [[] for _ in range(N)]
    for n, m in np.asarray(pairs).reshape(-1, 2).tolist():
        if n != m:
            rows[n].append(m)
            rows[m].append(n)
    rowptr, col = [0], []
    for r in rows:
        col += sorted(r)
        rowptr.append(len(col))
    return np.array(rowptr, dtype=np.int32), np.array(col, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ overlap sums and coefficients
def overlaps(boxes, offsets, w, pairs):
    """(G, abs-sums, terms): float64 [P] math.fsum of w_n w_m (exact products) over the pair's intersection, of |w_n w_m|, and the
    number of terms."""
    P = len(pairs)
    G, mag, terms = np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.int64)
    w = np.asarray(w, dtype=np.float32)
    for p, (n, m) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        box = intersection(boxes[n], boxes[m])
        if box is None:
            continue
        parts = []
        for k in (n, m):
            b = boxes[k]
            dense = w[int(offsets[k]):int(offsets[k + 1])].reshape(int(b[1] - b[0]), int(b[3] - b[2]), int(b[5] - b[4]))
            parts.append(dense[box[0] - b[0]:box[1] - b[0], box[2] - b[2]:box[3] - b[2], box[4] - b[4]:box[5] - b[4]].astype(np.float64).ravel())
        prod = (parts[0] * parts[1]).tolist()
        G[p], mag[p], terms[p] = math.fsum(prod), math.fsum(abs(v) for v in prod), len(prod)
    return G, mag, terms


def coefficients(G, pairs, rowptr, col, wsum, sizes):
    """val float64 [E] from G [P] in the order of pairs."""
    index = {(int(n), int(m)): p for p, (n, m) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist())}
    G, wsum = np.asarray(G, dtype=np.float64), np.asarray(wsum, dtype=np.float64)
    val = np.zeros(len(col))
    with np.errstate(all="ignore"):
        for n in range(len(rowptr) - 1):
            for e in range(int(rowptr[n]), int(rowptr[n + 1])):
                m = int(col[e])
                gnm, gmm = G[index[(min(n, m), max(n, m))]], G[index[(m, m)]]
                num = gnm * wsum[m]
                den = gmm * wsum[n]
                ok = sizes[n] > 0 and sizes[m] > 0 and gnm != 0.0 and gmm > 0.0 and wsum[n] > 0.0 and den > 0.0
                val[e] = num / den if ok else 0.0
    return val


def dense_matrix(rowptr, col, val):
    N = len(rowptr) - 1
    M = np.zeros((N, N))
    for n in range(N):
        for e in range(int(rowptr[n]), int(rowptr[n + 1])):
            M[n, int(col[e])] = val[e]
    return M


# ------------------------------------------------------------------------------------------------ the solve
def solve(F, rowptr, col, val, sizes, n_sweeps=64, tol=0.0, nonneg=True, trace=None):
    """(Fd float64 [N,T], sweeps int32 [T]).  trace: a list that receives the largest change of every sweep over the steps still
    running."""
    F = np.array(F, dtype=np.float64)
    N, T = F.shape
    live = np.asarray(sizes) > 0
    Fl = np.where(live[:, None], F, np.nan)
    f = Fl.copy()
    sweeps = np.zeros(T, dtype=np.int32)
    active = np.ones(T, dtype=bool)
    tol = np.float64(tol)
    with np.errstate(all="ignore"):
        for _ in range(int(n_sweeps)):
            idx = np.nonzero(active)[0]
            if not len(idx):
                break
            g = f[:, idx]
            ok = np.ones(len(idx), dtype=bool)
            largest = np.zeros(len(idx))
            for n in range(N):
                acc = np.zeros(len(idx))
                for e in range(int(rowptr[n]), int(rowptr[n + 1])):
                    c = val[e]
                    if c != 0.0:                                                   # skipped by selection; a NaN coefficient is not 0
                        acc = acc + c * g[int(col[e])]
                new = Fl[n, idx] - acc
                if nonneg:
                    new = np.where(new < 0.0, 0.0, new)
                new = np.where(np.isnan(new), np.nan, new)                         # one NaN: its sign is not arithmetic
                change = np.abs(new - g[n])
                if live[n]:                                                        # an empty footprint's row is NaN and is not iterated
                    ok &= change <= tol
                    largest = np.fmax(largest, change)
                g[n] = new
            f[:, idx] = g
            sweeps[idx] += 1
            active[idx[ok]] = False
            if trace is not None:
                trace.append(float(largest.max()))
    return f, sweeps


def demix(F, boxes, offsets, w, wsum, sizes, n_sweeps=64, tol=0.0, nonneg=True, G=None):
    """The whole restatement: (Fd, sweeps, (pairs, G, rowptr, col, val)); G: overlap sums to use instead of its own."""
    pairs = pairs_of(boxes)
    if G is None:
        G = overlaps(boxes, offsets, w, pairs)[0]
    rowptr, col = structure(pairs, len(boxes))
    val = coefficients(G, pairs, rowptr, col, wsum, sizes)
    Fd, sweeps = solve(F, rowptr, col, val, sizes, n_sweeps, tol, nonneg)
    return Fd, sweeps, (pairs, G, rowptr, col, val)


# ------------------------------------------------------------------------------------------------ the scene
SHAPE, FRAMES, SIGMA = FR.SHAPE, 80, FR.SIGMA
SEPARATIONS = ((0, 0, 5), (0, 3, 4), (1, 0, 4))
N_PAIRS = 3
PAIRED, ISOLATED = list(range(2 * N_PAIRS)), 2 * N_PAIRS


@functools.lru_cache(maxsize=None)
def scene(seed, bg, sep):
    """(stack float32 [T,D,H,W], centres int [7,3] (z, y, x), amplitudes [7,T]): footprints_ref.scene's recipe -- Gaussian blobs of
    sigma (1.2, 2, 2), amplitude 0.5 + U(0, 1) that is 0 with probability 0.6, the common background bg g(t) (1 + 0.5 sin(y / 9)
    cos(x / 7)), noise 0.05 -- with the blobs planted in three close pairs (2k, 2k + 1), the second `sep` from the first, plus one
    isolated blob (index 6); blobs of different pairs differ by at least (7, 12, 12) on some axis, so only partners' boxes meet.
    80 frames.  Do not write into the arrays."""
    rng = np.random.default_rng(seed)
    D, H, W = SHAPE
    groups = []
    while len(groups) < N_PAIRS + 1:
        c = tuple(int(rng.integers(FR.FACE[k], SHAPE[k] - FR.FACE[k] - sep[k])) for k in range(3))
        mine = [c] if len(groups) == N_PAIRS else [c, tuple(c[k] + sep[k] for k in range(3))]
        if all(any(abs(a[k] - o[k]) >= FR.APART[k] for k in range(3)) for g in groups for o in g for a in mine):
            groups.append(mine)
    centres = np.array([c for g in groups for c in g], dtype=np.int64)
    B = len(centres)
    amp = (0.5 + rng.random((B, FRAMES))) * (rng.random((B, FRAMES)) >= 0.6)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    stack = np.zeros((FRAMES, D, H, W))
    for n, (cz, cy, cx) in enumerate(centres):
        blob = np.exp(-0.5 * (((z - cz) / SIGMA[0]) ** 2 + ((y - cy) / SIGMA[1]) ** 2 + ((x - cx) / SIGMA[2]) ** 2))
        stack += amp[n][:, None, None, None] * blob
    g = np.cumsum(rng.normal(0.0, 0.3, FRAMES))
    g = g - g.min() + 0.5
    stack += bg * g[:, None, None, None] * (1.0 + 0.5 * np.sin(y / 9.0) * np.cos(x / 7.0))
    stack += 0.05 * rng.standard_normal(stack.shape)
    stack = stack.astype(np.float32)
    for a in (stack, centres, amp):
        a.setflags(write=False)
    return stack, centres, amp


@functools.lru_cache(maxsize=None)
def scene_traces(seed, bg, sep, thr=0.5, alpha=0.7):
    """The restatement from the scene to the traces: (geometry, (w, wsum, sizes), (F, Fnp, Fc), (Fd, sweeps), parts)."""
    x, centres, amp = scene(seed, bg, sep)
    geo = FR.Geometry(centres, SHAPE)
    corr, w, wsum, sizes = FR.footprints(x, geo, True, thr)
    F, Fnp, Fc, _ = FR.traces(x, geo, w, wsum, alpha)
    Fd, sweeps, parts = demix(F, geo.boxes, geo.offsets, w, wsum, sizes)
    return geo, (w, wsum, sizes), (F, Fnp, Fc), (Fd, sweeps), parts


def purpose(F, Fnp, Fc, Fd, amp, alpha=0.7):
    """(r_F, r_Fd, r_Fc, r_Fdc, cross_F, cross_Fd): the correlations of every neuron's trace with its own planted amplitude, and
    of the paired neurons' traces with their partner's (absolute)."""
    Fdc = np.where(np.isnan(Fnp), Fd, Fd - alpha * Fnp)
    own = [FR.trace_correlations(t, amp) for t in (F, Fd, Fc, Fdc)]
    partner = amp[[n ^ 1 for n in PAIRED]]
    cross = [np.abs(FR.trace_correlations(t[PAIRED], partner)) for t in (F, Fd)]
    return (*own, *cross)
