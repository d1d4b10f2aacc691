"""The numpy restatement of the neuron footprints and the scene their tests use.  No test functions here;
tests/test_footprints_cpu.py and tests/test_gpu_footprints.py import it.

Geometry (host, integers): boxes [c - r, c + r) and cores [c - core, c + core + 1) clipped, shells = the box grown by gap + annulus
minus the box grown by gap, both clipped by the volume, minus every voxel inside any box.  The state is ragged: box n's voxels in the
box's own (z, y, x) order at offsets[n].

    d_i(t) = (double)x_i(t) - (double)x_i(0)        e(t) = c(t) - c(0)        g(t) = u(t) - u(0)
    s1 += d   s2 += d d   sc += d e   su += d g     e1 += e   e2 += e e   g1 += g   g2 += g g   eg += e g       (t >= 1, from 0.0)
    v_a = max(s2_a - s1_a s1_a / T, 0)     r_ab = den > 0 ? (s_ab - s1_a s1_b / T) / den : 0,  den = sqrt(v_a v_b)
    q = (1 - r_ig r_ig)(1 - r_eg r_eg)     r = q > 0 ? (r_ie - r_ig r_eg) / sqrt(q) : 0         (without neuropil: r = r_ie)
    corr = (float)r     above = corr >= thr     footprint = the above voxels 6-connected inside the box to an above voxel of the core

Every sum is added to in time order by an explicit loop over t; every product and sum is one float64 numpy operation, rounded on its
own.  The traces' sums are math.fsum: the correctly rounded value of the exact sum."""
import functools
import math

import numpy as np

R, CORE, GAP, ANNULUS = (3, 5, 5), (1, 1, 1), (1, 2, 2), (2, 4, 4)


# ------------------------------------------------------------------------------------------------ geometry
def boxes_of(centres, shape, r=R):
    """int32 [N,6]: [c - r, c + r) per axis clipped by the volume; an empty range is written as (0, 0) (CWFA.roi_boxes)."""
    out = np.zeros((len(centres), 6), dtype=np.int32)
    for n, c in enumerate(centres):
        for k in range(3):
            lo, hi = max(0, int(c[k]) - r[k]), min(shape[k], int(c[k]) + r[k])
            if hi > lo:
                out[n, 2 * k], out[n, 2 * k + 1] = lo, hi
    return out


def cores_of(centres, boxes, core=CORE):
    """int32 [N,6]: [c - core, c + core + 1) clipped by the box; clipped away: the empty range at the box's lower corner."""
    out = np.zeros((len(centres), 6), dtype=np.int32)
    for n, c in enumerate(centres):
        rows = [(max(int(boxes[n, 2 * k]), int(c[k]) - core[k]), min(int(boxes[n, 2 * k + 1]), int(c[k]) + core[k] + 1)) for k in range(3)]
        if any(hi <= lo for lo, hi in rows):
            rows = [(int(boxes[n, 2 * k]),) * 2 for k in range(3)]
        out[n] = [v for row in rows for v in row]
    return out


def count(b):
    return int(b[1] - b[0]) * int(b[3] - b[2]) * int(b[5] - b[4])


def shells_of(boxes, shape, gap=GAP, annulus=ANNULUS):
    """(outer, inner) int32 [N,6]: the box grown by gap + annulus and by gap, clipped by the volume; all zero for an empty box."""
    outer, inner = np.zeros_like(boxes), np.zeros_like(boxes)
    for n, b in enumerate(boxes):
        if count(b) == 0:
            continue
        for k in range(3):
            for table, grow in ((outer, gap[k] + annulus[k]), (inner, gap[k])):
                table[n, 2 * k], table[n, 2 * k + 1] = max(0, int(b[2 * k]) - grow), min(shape[k], int(b[2 * k + 1]) + grow)
    return outer, inner


def offsets_of(boxes):
    return np.concatenate([[0], np.cumsum([count(b) for b in boxes])]).astype(np.int64)


def region(b):
    return (slice(int(b[0]), int(b[1])), slice(int(b[2]), int(b[3])), slice(int(b[4]), int(b[5])))


def occupancy(boxes, shape):
    occ = np.zeros(shape, dtype=np.uint8)
    for b in boxes:
        occ[region(b)] = 1
    return occ


def shell_mask(outer, inner, occ):
    """bool [D,H,W]: inside outer, outside inner, not occupied."""
    m = np.zeros(occ.shape, dtype=bool)
    m[region(outer)] = True
    m[region(inner)] = False
    return m & (occ == 0)


class Geometry:
    def __init__(self, centres, shape, r=R, core=CORE, gap=GAP, annulus=ANNULUS, boxes=None, cores=None):
        self.shape = tuple(shape)
        self.boxes = boxes_of(centres, shape, r) if boxes is None else np.asarray(boxes, dtype=np.int32).reshape(-1, 6)
        self.cores = cores_of(centres, self.boxes, core) if cores is None else np.asarray(cores, dtype=np.int32).reshape(-1, 6)
        self.outer, self.inner = shells_of(self.boxes, shape, gap, annulus)
        self.offsets = offsets_of(self.boxes)
        self.occ = occupancy(self.boxes, shape)
        self.N, self.V = len(self.boxes), int(self.offsets[-1])

    def shell(self, n):
        return shell_mask(self.outer[n], self.inner[n], self.occ)


# ------------------------------------------------------------------------------------------------ reference traces
def box_sums(x, boxes):
    """float64 [N,T]: the plain sums over the boxes (any accurate order will do: they are an input of the accumulation)."""
    x = np.asarray(x)
    return np.array([[math.fsum(x[t][region(b)].astype(np.float64).ravel().tolist()) for t in range(x.shape[0])] for b in boxes]).reshape(
        len(boxes), x.shape[0])


def shell_sums(x, geo):
    """(sums float64 [N,T] by math.fsum, abs-sums, counts)."""
    x = np.asarray(x)
    T = x.shape[0]
    sums, mags, counts = np.zeros((geo.N, T)), np.zeros((geo.N, T)), np.zeros(geo.N, dtype=np.int32)
    for n in range(geo.N):
        m = geo.shell(n)
        counts[n] = m.sum()
        for t in range(T):
            v = x[t][m].astype(np.float64).tolist()
            sums[n, t], mags[n, t] = math.fsum(v), math.fsum(abs(a) for a in v)
    return sums, mags, counts


def weighted_sums(x, boxes, offsets, w=None):
    """(sums, abs-sums, terms): float64 [N,T] math.fsum of w_i x_i (exact products) over every box, of |w_i x_i|, and the number of
    terms [N]."""
    x = np.asarray(x)
    T, N = x.shape[0], len(boxes)
    sums, mags, terms = np.zeros((N, T)), np.zeros((N, T)), np.zeros(N, dtype=np.int64)
    for n, b in enumerate(boxes):
        terms[n] = count(b)
        wn = None if w is None else np.asarray(w[int(offsets[n]):int(offsets[n + 1])], dtype=np.float64)
        for t in range(T):
            v = x[t][region(b)].astype(np.float64).ravel()
            v = (v if wn is None else wn * v).tolist()
            sums[n, t], mags[n, t] = math.fsum(v), math.fsum(abs(a) for a in v)
    return sums, mags, terms


# ------------------------------------------------------------------------------------------------ accumulation
def accumulate(x, geo, c, u=None, state=None):
    """(x0 float32 [V], acc float64 [4,V], ref float64 [N,7]) after the chunk x [T',D,H,W] with the reference traces c, u [N,T'];
    state: what an earlier chunk returned (None: this is the first chunk, whose first volume only initialises)."""
    x = np.asarray(x, dtype=np.float32)
    c = np.asarray(c, dtype=np.float64).reshape(geo.N, x.shape[0])
    u = None if u is None else np.asarray(u, dtype=np.float64).reshape(geo.N, x.shape[0])
    first = state is None
    if first:
        x0, acc, ref = np.zeros(geo.V, dtype=np.float32), np.zeros((4, geo.V)), np.zeros((geo.N, 7))
    else:
        x0, acc, ref = (a.copy() for a in state)
    with np.errstate(invalid="ignore", over="ignore"):
        for n, b in enumerate(geo.boxes):
            lo, hi = int(geo.offsets[n]), int(geo.offsets[n + 1])
            X = x[(slice(None), *region(b))].reshape(x.shape[0], hi - lo)
            if first:
                x0[lo:hi] = X[0]
                ref[n, 0] = c[n, 0]
                ref[n, 1] = 0.0 if u is None else u[n, 0]
            xd = x0[lo:hi].astype(np.float64)
            s1, s2, sc, su = (acc[k, lo:hi].copy() for k in range(4))
            e1, e2, g1, g2, eg = ref[n, 2:]
            for t in range(1 if first else 0, x.shape[0]):
                d = X[t].astype(np.float64) - xd
                e = c[n, t] - ref[n, 0]
                s1 = s1 + d
                s2 = s2 + d * d
                sc = sc + d * e
                e1 = e1 + e
                e2 = e2 + e * e
                if u is not None:
                    g = u[n, t] - ref[n, 1]
                    su = su + d * g
                    g1 = g1 + g
                    g2 = g2 + g * g
                    eg = eg + e * g
            acc[0, lo:hi], acc[1, lo:hi], acc[2, lo:hi], acc[3, lo:hi] = s1, s2, sc, su
            ref[n, 2:] = e1, e2, g1, g2, eg
    return x0, acc, ref


def _var(s1, s2, T):
    v = s2 - s1 * s1 / T
    return np.where(v < 0.0, 0.0, v)


def _r(sab, sa, sb, va, vb, T):
    den = np.sqrt(va * vb)
    cov = sab - sa * sb / T
    ok = den > 0.0
    return np.where(ok, cov / np.where(ok, den, 1.0), 0.0)


def pair_correlations(acc, ref, geo, T):
    """(r_ie [V], r_ig [V], r_eg [N]) in float64."""
    T = np.float64(T)
    rie, rig, reg = np.zeros(geo.V), np.zeros(geo.V), np.zeros(geo.N)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for n in range(geo.N):
            lo, hi = int(geo.offsets[n]), int(geo.offsets[n + 1])
            e1, e2, g1, g2, eg = (np.float64(v) for v in ref[n, 2:])
            ve, vg = _var(e1, e2, T), _var(g1, g2, T)
            reg[n] = _r(eg, e1, g1, ve, vg, T)
            s1, s2, sc, su = acc[:, lo:hi]
            vi = _var(s1, s2, T)
            rie[lo:hi] = _r(sc, s1, e1, vi, ve, T)
            rig[lo:hi] = _r(su, s1, g1, vi, vg, T)
    return rie, rig, reg


def partial_correlations(acc, ref, geo, T):
    """r [V] in float64: the correlation of voxel and seed given the neuropil trace."""
    rie, rig, reg = pair_correlations(acc, ref, geo, T)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rg = np.repeat(reg, np.diff(geo.offsets))
        q = (1.0 - rig * rig) * (1.0 - rg * rg)
        ok = q > 0.0
        return np.where(ok, (rie - rig * rg) / np.sqrt(np.where(ok, q, 1.0)), 0.0)


def correlate(acc, ref, geo, T, neuropil=True):
    """corr float32 [V]."""
    r = partial_correlations(acc, ref, geo, T) if neuropil else pair_correlations(acc, ref, geo, T)[0]
    return r.astype(np.float32)


# ------------------------------------------------------------------------------------------------ selection
def fill(above, seed):
    """The voxels of `above` 6-connected to a voxel of `seed & above`: iterated 6-neighbour dilation ANDed with `above`."""
    cur = above & seed
    while True:
        grown = cur.copy()
        for ax in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            grown[tuple(hi)] |= cur[tuple(lo)]
            grown[tuple(lo)] |= cur[tuple(hi)]
        grown &= above
        if np.array_equal(grown, cur):
            return cur
        cur = grown


def select(corr, geo, thr):
    """(w float32 [V], wsum float64 [N], sizes int32 [N])."""
    corr = np.asarray(corr, dtype=np.float32)
    thr = np.float32(thr)
    w, wsum, sizes = np.zeros(geo.V, dtype=np.float32), np.zeros(geo.N), np.zeros(geo.N, dtype=np.int32)
    for n, (b, co) in enumerate(zip(geo.boxes, geo.cores)):
        lo, hi = int(geo.offsets[n]), int(geo.offsets[n + 1])
        dims = (int(b[1] - b[0]), int(b[3] - b[2]), int(b[5] - b[4]))
        with np.errstate(invalid="ignore"):
            above = (corr[lo:hi] >= thr).reshape(dims)
        seed = np.zeros(dims, dtype=bool)
        seed[int(co[0] - b[0]):int(co[1] - b[0]), int(co[2] - b[2]):int(co[3] - b[2]), int(co[4] - b[4]):int(co[5] - b[4])] = True
        inside = fill(above, seed).ravel()
        w[lo:hi] = np.where(inside, corr[lo:hi], np.float32(0.0))
        sizes[n] = inside.sum()
        total = 0.0
        for v in w[lo:hi].astype(np.float64).tolist():                    # box-linear order, from 0.0
            total = total + v
        wsum[n] = total
    return w, wsum, sizes


def dense(a, geo, n):
    b = geo.boxes[n]
    return a[int(geo.offsets[n]):int(geo.offsets[n + 1])].reshape(int(b[1] - b[0]), int(b[3] - b[2]), int(b[5] - b[4]))


# ------------------------------------------------------------------------------------------------ traces
def traces(x, geo, w, wsum, alpha=0.7, neuropil=True):
    """(F, Fnp, Fc, bound): float64 [N,T]; bound: what a float64 tree sum of the same terms may differ from F by (module docstring of
    tests/test_gpu_footprints.py)."""
    s, mag, terms = weighted_sums(x, geo.boxes, geo.offsets, w)
    with np.errstate(invalid="ignore", divide="ignore"):
        F = s / wsum[:, None]
        bound = (terms[:, None] + 2) * 2.0 ** -53 * mag / wsum[:, None]
        if neuropil:
            ss, _, counts = shell_sums(x, geo)
            Fnp = ss / counts.astype(np.float64)[:, None]
        else:
            Fnp = np.full_like(F, np.nan)
        Fc = np.where(np.isnan(Fnp), F, F - alpha * Fnp)
    return F, Fnp, Fc, bound


def footprints(x, geo, neuropil=True, thr=0.5, chunk=None):
    """(corr, w, wsum, sizes) of the whole restatement on the stack x, with its own reference traces."""
    x = np.asarray(x)
    c = box_sums(x, geo.cores)
    u = shell_sums(x, geo)[0] if neuropil else None
    state = None
    step = x.shape[0] if chunk is None else chunk
    for t in range(0, x.shape[0], step):
        state = accumulate(x[t:t + step], geo, c[:, t:t + step], None if u is None else u[:, t:t + step], state)
    corr = correlate(state[1], state[2], geo, x.shape[0], neuropil)
    return (corr, *select(corr, geo, thr))


# ------------------------------------------------------------------------------------------------ the scene
SHAPE, FRAMES, BLOBS, SIGMA = (14, 56, 64), 60, 6, (1.2, 2.0, 2.0)
FACE, APART = (4, 8, 8), (7, 12, 12)


@functools.lru_cache(maxsize=None)
def scene(seed, bg):
    """(stack float32 [T,D,H,W], centres int [N,3] (z, y, x), amplitudes [N,T]): N = 6 Gaussian blobs of sigma (1.2, 2, 2) whose
    centres lie at least (4, 8, 8) from the faces and differ pairwise by at least (7, 12, 12) on some axis; per time step an amplitude
    0.5 + U(0, 1) that is 0 with probability 0.6; a common background bg g(t) (1 + 0.5 sin(y / 9) cos(x / 7)), g a cumulative sum of
    N(0, 0.3) shifted so that its minimum is 0.5; noise 0.05 N(0, 1) on every voxel.  Do not write into the arrays."""
    rng = np.random.default_rng(seed)
    D, H, W = SHAPE
    centres = []
    while len(centres) < BLOBS:
        c = tuple(int(rng.integers(FACE[k], SHAPE[k] - FACE[k])) for k in range(3))
        if all(any(abs(c[k] - o[k]) >= APART[k] for k in range(3)) for o in centres):
            centres.append(c)
    centres = np.array(centres, dtype=np.int64)
    amp = (0.5 + rng.random((BLOBS, FRAMES))) * (rng.random((BLOBS, FRAMES)) >= 0.6)
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


def box_means(x, boxes):
    return box_sums(x, boxes) / np.array([max(count(b), 1) for b in boxes], dtype=np.float64)[:, None]


def trace_correlations(tr, amp):
    return np.array([np.corrcoef(tr[n], amp[n])[0, 1] for n in range(len(amp))])


# ------------------------------------------------------------------------------------------------ hand-made cases
def small_case(T=40, seed=3):
    """A [T,3,6,7] stack with a mean of 3, one box that is the whole volume, and an external neuropil trace mixed into every voxel."""
    rng = np.random.default_rng(seed)
    shape = (3, 6, 7)
    common = rng.standard_normal(T)
    x = (3.0 + rng.standard_normal((T, *shape)) + 0.8 * common[:, None, None, None]).astype(np.float32)
    geo = Geometry([(1, 3, 3)], shape, r=(5, 5, 5))
    c = box_sums(x, geo.cores)
    u = (10.0 * common + rng.standard_normal(T))[None, :]
    return x, geo, c, u


def serpentine():
    """A 1 x 9 x 9 map whose above voxels are one path of width 1 from the centre outwards."""
    a = np.zeros((1, 9, 9), dtype=bool)
    for row in range(0, 9, 2):
        a[0, row, :] = True
    for k, row in enumerate(range(1, 9, 2)):
        a[0, row, 8 if k % 2 == 0 else 0] = True
    return a


def box_case(above, core, value=0.75):
    """(geometry, corr, expected mask) of one box of above's shape with corr = value where above, 0.25 elsewhere."""
    dims = above.shape
    boxes = [[0, dims[0], 0, dims[1], 0, dims[2]]]
    geo = Geometry(None, dims, boxes=boxes, cores=[core])
    corr = np.where(above, np.float32(value), np.float32(0.25)).astype(np.float32).ravel()
    return geo, corr


def _island():
    a = np.zeros((3, 7, 7), dtype=bool)
    a[1, 2:5, 2:5] = True
    a[1, 6, 6] = a[0, 0, 0] = True                                             # not connected to the core
    want = a.copy()
    want[1, 6, 6] = want[0, 0, 0] = False
    return a, [1, 2, 3, 4, 3, 4], want


def _diagonal():
    a = np.zeros((3, 7, 7), dtype=bool)
    a[1, 3, 3] = a[1, 4, 4] = a[2, 4, 3] = a[0, 2, 2] = True                     # edge and corner contacts only
    want = np.zeros_like(a)
    want[1, 3, 3] = True
    return a, [1, 2, 3, 4, 3, 4], want


def _core_below():
    a = np.ones((3, 7, 7), dtype=bool)
    a[1, 3, 3] = False
    return a, [1, 2, 3, 4, 3, 4], np.zeros_like(a)


def _serp():
    a = serpentine()
    return a, [0, 1, 4, 5, 4, 5], a.copy()


def fill_case(name):
    return {"island": _island, "diagonal": _diagonal, "core_below": _core_below, "serpentine": _serp}[name]()


def special_case():
    """(stack [6,3,6,7], geometry, c, u, planted): one box, the whole volume; a constant voxel, NaN, +inf, -inf inside a series and
    +inf as a first sample."""
    x, geo, c, u = small_case(T=6, seed=4)
    x = x.copy()
    planted = {(1, 1, 1): ("const", 2.5), (1, 1, 5): (3, np.nan), (1, 4, 2): (2, np.inf), (2, 4, 5): (4, -np.inf), (0, 5, 4): (0, np.inf)}
    for (z, y, xx), (t, v) in planted.items():
        if t == "const":
            x[:, z, y, xx] = v
        else:
            x[t, z, y, xx] = v
    return x, geo, c, u, [np.ravel_multi_index(k, geo.shape) for k in planted]
