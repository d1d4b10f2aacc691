"""The numpy restatement of the streaming local-correlation map and the scene its end-to-end tests use.  No test
functions here; tests/test_corrmap_cpu.py and tests/test_gpu_corrmap.py import it.

    d_i(t) = (double)x_i(t) - (double)x_i(0)
    s1_i = sum_{t>=1} d_i(t)      s2_i = sum_{t>=1} d_i(t) d_i(t)      cc[k][i] = sum_{t>=1} d_i(t) d_j(t),  j = i + o_k
    v_i = max(s2_i - s1_i s1_i / N, 0)    cov = c - s1_i s1_j / N    den = sqrt(v_i v_j)    r = den > 0 ? cov / den : 0
    score_i = (float)(sum of r over the in-volume offsets in lexicographic order / their number), 0 where there are none

Every sum starts from 0.0 and is added to in time order by an explicit loop over t; every product and sum is one float64 numpy
operation, rounded on its own.  Neighbours are taken by slicing coordinates, so nothing wraps around a row or a plane."""
import functools

import numpy as np

import neurons_ref


def offsets(neighbours):
    """All offsets (dz, dy, dx) of the neighbourhood, in lexicographic order."""
    cube = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
    if neighbours == 26:
        return cube
    if neighbours == 8:
        return [o for o in cube if o[0] == 0]
    if neighbours == 6:
        return [o for o in cube if abs(o[0]) + abs(o[1]) + abs(o[2]) == 1]
    raise ValueError(f"neighbours is 6, 8 or 26, got {neighbours!r}")


def forward(neighbours):
    """The lexicographically positive half, in lexicographic order: o_0 .. o_{K-1}."""
    return [o for o in offsets(neighbours) if o > (0, 0, 0)]


def pair(shape, o):
    """(lo, hi): slices of a [.., D, H, W] array such that a[lo] holds the voxels i whose neighbour j = i + o is inside the volume and
    a[hi] holds those neighbours, voxel for voxel.  o is a forward or a backward offset."""
    lo, hi = [], []
    for n, d in zip(shape, o):
        lo.append(slice(max(0, -d), max(n - max(0, d), max(0, -d))))
        hi.append(slice(max(0, d), max(n - max(0, -d), max(0, d))))
    return (Ellipsis, *lo), (Ellipsis, *hi)


def accumulate(x, neighbours):
    """(x0 float32, s1, s2 float64 [D,H,W], cc float64 [K,D,H,W]) of the stack x [N,D,H,W] (float32)."""
    x = np.asarray(x, dtype=np.float32)
    fw = forward(neighbours)
    shape = x.shape[1:]
    x0 = x[0].copy()
    s1, s2, cc = np.zeros(shape), np.zeros(shape), np.zeros((len(fw), *shape))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, x.shape[0]):
            d = x[t].astype(np.float64) - x0.astype(np.float64)
            s1 = s1 + d
            s2 = s2 + d * d
            for k, o in enumerate(fw):
                lo, hi = pair(shape, o)
                cc[k][lo] = cc[k][lo] + d[lo] * d[hi]
    return x0, s1, s2, cc


def pair_correlations(s1, s2, cc, N, neighbours):
    """{offset: r}: for every offset of the whole neighbourhood an array [D,H,W] holding r_ij at the voxels whose neighbour is inside
    the volume (0 elsewhere), and `inside`, the boolean mask of those voxels, as {offset: mask}."""
    fw = forward(neighbours)
    shape = s1.shape
    N = np.float64(N)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = s2 - s1 * s1 / N
        v = np.where(v < 0.0, 0.0, v)
        rs, inside = {}, {}
        for o in offsets(neighbours):
            lo, hi = pair(shape, o)
            if o > (0, 0, 0):
                c = cc[fw.index(o)][lo]                                  # kept at the lower voxel: i itself
            else:
                c = cc[fw.index(tuple(-a for a in o))][hi]               # kept at the lower voxel: the neighbour j = i + o
            cov = c - s1[lo] * s1[hi] / N
            den = np.sqrt(v[lo] * v[hi])
            r = np.zeros(shape)
            r[lo] = np.where(den > 0.0, cov / np.where(den > 0.0, den, 1.0), 0.0)
            m = np.zeros(shape, dtype=bool)
            m[lo] = True
            rs[o], inside[o] = r, m
    return rs, inside


def finish(s1, s2, cc, N, neighbours):
    """(score float32 [D,H,W], n int [D,H,W])."""
    rs, inside = pair_correlations(s1, s2, cc, N, neighbours)
    total, n = np.zeros(s1.shape), np.zeros(s1.shape, dtype=np.int64)
    for o in offsets(neighbours):                                        # lexicographic order, added to 0.0
        total = np.where(inside[o], total + rs[o], total)
        n += inside[o]
    score = np.where(n > 0, total / np.maximum(n, 1), 0.0).astype(np.float32)
    return score, n


def score(x, neighbours):
    x0, s1, s2, cc = accumulate(x, neighbours)
    return finish(s1, s2, cc, x.shape[0], neighbours)[0]


@functools.lru_cache(maxsize=None)
def special_stack():
    """(clean, planted, coords): a random [6,3,7,9] stack, and the same with one constant voxel, a NaN, +inf and -inf inside a series
    and +inf as a first sample, no two of them neighbours; coords: where they are.  Do not write into the arrays."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((6, 3, 7, 9)).astype(np.float32)
    planted = {(1, 1, 1): ("const", 2.5), (1, 1, 5): (3, np.nan), (1, 4, 2): (2, np.inf), (1, 4, 6): (4, -np.inf), (1, 5, 4): (0, np.inf)}
    y = x.copy()
    for (z, yy, xx), (t, v) in planted.items():
        if t == "const":
            y[:, z, yy, xx] = v
        else:
            y[t, z, yy, xx] = v
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, tuple(planted)


def touched(coords, shape, neighbours):
    """The boolean mask of the voxels at `coords` and of their in-volume neighbours."""
    mask = np.zeros(shape, dtype=bool)
    for c in coords:
        mask[c] = True
        for o in offsets(neighbours):
            j = tuple(a + b for a, b in zip(c, o))
            if all(0 <= a < n for a, n in zip(j, shape)):
                mask[j] = True
    return mask


# what the end-to-end tests fix: Gaussian noise on every voxel, isolated voxels of independent high-variance noise, the absolute
# threshold on the correlation map, and the detector's window and margin
NOISE, HOT, HOT_SIGMA, THR, DIST, MARGIN = 0.1, 40, 1.5, 0.5, (5, 9, 9), (3, 5, 5)


@functools.lru_cache(maxsize=None)
def scene_hot(seed, noise=NOISE, hot=HOT, hot_sigma=HOT_SIGMA):
    """(stack float32 [T,D,H,W], centres): neurons_ref.scene's blobs (24 of them in 24 x 96 x 112, T = 40, whose centres lie at least
    (3, 5, 5) from every face) with Gaussian noise of sigma `noise` on every voxel and `hot` isolated voxels carrying independent
    noise of sigma `hot_sigma`: voxels that fluctuate more than any neuron and with nothing around them.  Do not write into it."""
    base, centres = neurons_ref.scene(seed)
    rng = np.random.default_rng(1000 + seed)
    stack = base.astype(np.float64) + noise * rng.standard_normal(base.shape)
    T, D, H, W = base.shape
    for _ in range(hot):
        z, y, x = int(rng.integers(0, D)), int(rng.integers(0, H)), int(rng.integers(0, W))
        stack[:, z, y, x] += hot_sigma * rng.standard_normal(T)
    stack = stack.astype(np.float32)
    stack.setflags(write=False)
    return stack, centres


@functools.lru_cache(maxsize=None)
def scene_peaks(seed):
    """(zyx, scores, total) of the restatement's 26-neighbour map of scene_hot(seed) at THR, DIST, MARGIN: what the device must find."""
    stack, _ = scene_hot(seed)
    return neurons_ref.local_maxima(score(stack, 26), THR, DIST, MARGIN)
