"""CPU: the demixing of overlapping footprints without a GPU -- the host pair enumeration against the O(N^2)
definition, the CSR structure, the numpy restatement tests/demix_ref.py against a dense solve, its invariants (an isolated neuron's
bits, component independence, special values, tol / n_sweeps), the purpose of the feature on the scene with close pairs, the argument
validation of the entry points through the built library, and the refusals the Python layer decides before any device work.

The dense solve.  Gauss-Seidel on (I + M) f = F contracts the error by a factor rho per sweep; on the cases here the largest change of
a sweep falls to 0.01 - 0.2 of the sweep before (printed; the chains' coefficients are 0.5 - 1.5 times 0.15 - 0.3, and rho is about the
product of two of them), and the iteration stops at a sweep that changes nothing (tol = 0), so what is left is rounding: each of the
k <= 4 products and sums of a row is off by at most 2^-53 of a magnitude <= |F|_max, amplified by at most 1 / (1 - rho) <= 1.34 on the
way to the fixpoint, and np.linalg.solve is backward stable with cond(I + M) <= 4 here.  The bound used is 64 * 2^-53 * |F|_max: a
order above that estimate, thirteen orders below the coefficients."""
import ctypes
import time

import numpy as np
import pytest
import torch

import demix_ref as D
import footprints_ref as FR


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


def host(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ pairs and structure
def random_boxes(N=130, seed=5, shape=(5, 10, 12), most=(4, 7, 8)):
    rng = np.random.default_rng(seed)
    lo = np.stack([rng.integers(0, n, N) for n in shape], axis=1)
    hi = np.minimum(lo + np.stack([rng.integers(0, m + 1, N) for m in most], axis=1), shape)
    boxes = np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1], lo[:, 2], hi[:, 2]], axis=1).astype(np.int32)
    boxes[(hi <= lo).any(1)] = 0
    return boxes


PAIR_CASES = {
    "disjoint": [[0, 2, 0, 2, 0, 2], [3, 5, 0, 2, 0, 2], [0, 2, 5, 6, 0, 2]],
    "touching": [[0, 2, 0, 2, 0, 2], [2, 4, 0, 2, 0, 2], [0, 2, 2, 4, 0, 2], [1, 3, 1, 3, 1, 3]],
    "nested": [[0, 6, 0, 10, 0, 10], [2, 4, 3, 5, 3, 5], [2, 3, 3, 4, 3, 4], [0, 6, 0, 10, 0, 10]],
    "clipped": [[0, 3, 0, 5, 0, 5], [0, 3, 3, 8, 0, 5], [1, 4, 0, 2, 4, 9], [2, 3, 4, 5, 4, 5]],
    "empty": [[0, 2, 0, 2, 0, 2], [0, 0, 0, 0, 0, 0], [1, 3, 1, 3, 1, 3], [1, 1, 0, 2, 0, 2]],
    "none": np.zeros((0, 6), dtype=np.int32),
    "one": [[1, 3, 1, 3, 1, 3]],
    "one_empty": [[0, 0, 0, 0, 0, 0]],
    "random130": random_boxes(),
}


@pytest.mark.parametrize("name", list(PAIR_CASES))
def test_pairs_are_the_quadratic_definition_and_the_structure_is_sorted_and_symmetric(name):
    from cwfa_amd import ops
    boxes = np.asarray(PAIR_CASES[name], dtype=np.int32).reshape(-1, 6)
    N = len(boxes)
    want = D.pairs_of(boxes)
    got = ops.footprint_pairs(boxes)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    assert sum(1 for n, m in got.tolist() if n == m) == N, "the diagonal of every box, empty or not"
    rowptr, col = ops.demix_structure(got, N)
    wr, wc = D.structure(want, N)
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and np.array_equal(rowptr, wr) and np.array_equal(col, wc)
    entries = set()
    for n in range(N):
        row = col[rowptr[n]:rowptr[n + 1]].tolist()
        assert row == sorted(set(row)) and n not in row, "ascending, no repeats, no diagonal"
        entries |= {(n, m) for m in row}
    assert entries == {(m, n) for n, m in entries}, "the pattern is symmetric"
    assert len(entries) == 2 * (len(got) - N)
    if name == "touching":
        assert [tuple(p) for p in got.tolist() if p[0] != p[1]] == [(0, 3), (1, 3), (2, 3)], "faces that touch share no voxel"
    if name == "random130":
        assert len(got) > 4 * N and (np.diff(rowptr) == 0).any(), "many pairs, and boxes that meet nobody"


def test_pairs_of_4096_boxes_take_well_under_a_second():
    from cwfa_amd import ops
    z, y, x = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    c = np.stack([3 + 4 * z.ravel(), 5 + 7 * y.ravel(), 5 + 7 * x.ravel()], axis=1)
    boxes = FR.boxes_of(c, (80, 130, 130))
    t0 = time.perf_counter()
    pairs = ops.footprint_pairs(boxes)
    took = time.perf_counter() - t0
    # interior boxes of 6 x 10 x 10 on a 4 x 7 x 7 lattice meet 3 x 3 x 3 - 1 = 26 neighbours
    assert len(boxes) == 4096 and np.bincount(np.concatenate([pairs[:, 0], pairs[:, 1]])).max() == 28
    assert took < 1.0, f"{took:.2f} s"
    rowptr, col = ops.demix_structure(pairs, 4096)
    assert int(np.diff(rowptr).max()) == 26 and len(col) == 2 * (len(pairs) - 4096)


# ------------------------------------------------------------------------------------------------ hand-made systems
def chain(N, c=0.2, empty=()):
    """A chain of N neurons coupled to their neighbours with coefficients around c: (rowptr, col, val, sizes)."""
    pairs = np.array(sorted([(n, n) for n in range(N)] + [(n, n + 1) for n in range(N - 1)]), dtype=np.int32)
    rowptr, col = D.structure(pairs, N)
    val = c * (0.5 + np.random.default_rng(N).random(len(col)))
    sizes = np.ones(N, dtype=np.int32)
    for n in empty:
        sizes[n] = 0
        val[rowptr[n]:rowptr[n + 1]] = 0.0
        val[col == n] = 0.0
    return rowptr, col, val, sizes


def traces_for(N, T=9, seed=0):
    return 1.0 + np.random.default_rng(seed).random((N, T))


def test_the_restatement_reaches_the_dense_solution():
    for N, c in ((2, 0.3), (7, 0.2), (40, 0.15)):
        rowptr, col, val, sizes = chain(N, c)
        F = traces_for(N)
        trace = []
        Fd, sweeps = D.solve(F, rowptr, col, val, sizes, n_sweeps=64, tol=0.0, nonneg=False, trace=trace)
        want = np.linalg.solve(np.eye(N) + D.dense_matrix(rowptr, col, val), F)
        err, bound = np.abs(Fd - want).max(), 64 * 2.0 ** -53 * np.abs(F).max()
        ratios = [b / a for a, b in zip(trace[:-1], trace[1:]) if a > 1e-12]
        print(f"N = {N}: {sweeps.max()} sweeps, contraction {min(ratios):.3f} - {max(ratios):.3f}, error {err:.2e}, bound {bound:.2e}")
        assert sweeps.max() < 64 and trace[-1] == 0.0, "a fixpoint, not the sweep limit"
        assert max(ratios) < 0.25 and err <= bound
    _, _, (F, _, _), (Fd, sweeps), (pairs, G, rowptr, col, val) = D.scene_traces(0, 0.05, D.SEPARATIONS[0])
    sol = np.linalg.solve(np.eye(7) + D.dense_matrix(rowptr, col, val), F)
    assert (sol > 0).all(), "the projection is idle on this scene: the projected fixpoint is the linear solution"
    assert np.abs(Fd - sol).max() <= 64 * 2.0 ** -53 * np.abs(F).max() and sweeps.max() <= 12


def test_an_isolated_neuron_keeps_its_bits():
    rowptr, col, val, sizes = chain(5)
    rowptr = np.concatenate([rowptr, [rowptr[-1]]]).astype(np.int32)              # a sixth neuron without entries
    sizes = np.concatenate([sizes, [1]]).astype(np.int32)
    F = traces_for(6) * np.array([1, 1, 1, 1, 1, -1])[:, None]
    F[5, 3] = -0.0
    Fd, _ = D.solve(F, rowptr, col, val, sizes, nonneg=False)
    assert same_bits(Fd[5], F[5]) and not same_bits(Fd[:5], F[:5])
    Fd, _ = D.solve(F, rowptr, col, val, sizes, nonneg=True)
    assert same_bits(Fd[5], np.where(F[5] < 0, 0.0, F[5])) and np.signbit(Fd[5, 3]), "only the projection touches it; -0.0 is not < 0"


def test_components_do_not_depend_on_which_comes_first():
    """Three components (a chain of 4, a pair, a single) in every order: each row's bits are those of its component alone."""
    parts = [chain(4, 0.3), chain(2, 0.4), chain(1)]
    Fs = [traces_for(4, seed=1), traces_for(2, seed=2), traces_for(1, seed=3)]
    alone = [D.solve(F, *p, tol=1e-9)[0] for F, p in zip(Fs, parts)]
    alone_sweeps = [D.solve(F, *p, tol=1e-9)[1] for F, p in zip(Fs, parts)]
    for order in ((0, 1, 2), (2, 1, 0), (1, 0, 2), (1, 2, 0)):
        rowptr, col, val, sizes, base = [0], [], [], [], 0
        for k in order:
            rp, c, v, s = parts[k]
            col += (c + base).tolist()
            val += v.tolist()
            rowptr += (rp[1:] + rowptr[-1]).tolist()
            sizes += s.tolist()
            base += len(s)
        got, sweeps = D.solve(np.concatenate([Fs[k] for k in order]), np.array(rowptr), np.array(col), np.array(val), np.array(sizes), tol=0.0)
        want = np.concatenate([D.solve(Fs[k], *parts[k], tol=0.0)[0] for k in order])
        assert same_bits(got, want), order
        assert np.array_equal(sweeps, np.maximum.reduce([D.solve(Fs[k], *parts[k], tol=0.0)[1] for k in order]))
    assert all(a.shape == F.shape for a, F in zip(alone, Fs)) and all((s >= 1).all() for s in alone_sweeps)


def test_special_values():
    # an empty footprint between two neurons: nothing passes through it, its row is NaN, the others see only their own G
    rowptr, col, val, sizes = chain(3, 0.3, empty=(1,))
    F = traces_for(3)
    F[1] = np.nan
    Fd, sweeps = D.solve(F, rowptr, col, val, sizes, tol=0.0)
    assert np.isnan(Fd[1]).all() and same_bits(Fd[0], F[0]) and same_bits(Fd[2], F[2]) and (sweeps == 1).all()
    F[1] = 5.0                                                                    # whatever F holds there
    assert np.isnan(D.solve(F, rowptr, col, val, sizes)[0][1]).all()
    # boxes: 0 and 2 overlap each other and the empty footprint 1
    boxes = np.array([[0, 4, 0, 4, 0, 6], [0, 4, 0, 4, 2, 8], [0, 4, 0, 4, 4, 10]], dtype=np.int32)
    off = FR.offsets_of(boxes)
    w = np.random.default_rng(1).uniform(0.5, 1.0, off[-1]).astype(np.float32)
    w[off[1]:off[2]] = 0.0
    wsum = np.array([w[off[k]:off[k + 1]].astype(np.float64).sum() for k in range(3)])
    sizes = np.array([96, 0, 96], dtype=np.int32)
    Fd, _, (pairs, G, rowptr, col, val) = D.demix(traces_for(3), boxes, off, w, wsum, sizes)
    M = D.dense_matrix(rowptr, col, val)
    assert pairs.tolist() == [[0, 0], [0, 1], [0, 2], [1, 1], [1, 2], [2, 2]] and G[1] == 0.0 and G[3] == 0.0 and G[4] == 0.0
    assert not M[1].any() and not M[:, 1].any() and M[0, 2] > 0 and M[2, 0] > 0
    assert M[0, 2] == (G[2] * wsum[2]) / (G[5] * wsum[0]) and M[2, 0] == (G[2] * wsum[0]) / (G[0] * wsum[2])
    # a NaN in F stays inside its component, at its time step
    rp, c, v, s = chain(2, 0.3)
    rowptr = np.concatenate([rp, rp[1:] + rp[-1]])
    col, val, sizes = np.concatenate([c, c + 2]), np.concatenate([v, v]), np.ones(4, dtype=np.int32)
    F = traces_for(4)
    clean = D.solve(F, rowptr, col, val, sizes, n_sweeps=20)
    F[0, 4] = np.nan
    Fd, sweeps = D.solve(F, rowptr, col, val, sizes, n_sweeps=20)
    assert np.isnan(Fd[:2, 4]).all() and sweeps[4] == 20, "a NaN change never ends a time step"
    keep = np.ones(F.shape, dtype=bool)
    keep[:2, 4] = False
    assert not np.isnan(Fd[keep]).any() and np.array_equal(bits(Fd)[keep], bits(clean[0])[keep])
    assert np.array_equal(np.delete(sweeps, 4), np.delete(clean[1], 4))
    # the projection
    F = np.array([[1.0, 0.1], [1.0, 2.0]])
    rowptr, col, val, sizes = np.array([0, 1, 2]), np.array([1, 0]), np.array([0.5, 0.5]), np.ones(2, dtype=np.int32)
    free = D.solve(F, rowptr, col, val, sizes, nonneg=False)[0]
    proj = D.solve(F, rowptr, col, val, sizes, nonneg=True)[0]
    assert free[0, 1] < 0 and proj[0, 1] == 0.0 and proj[1, 1] == 2.0 and same_bits(free[:, 0], proj[:, 0])


def test_tol_and_n_sweeps():
    rowptr, col, val, sizes = chain(6, 0.3)
    F = traces_for(6, T=12) * np.linspace(1e-3, 1e3, 12)[None, :]                 # steps of very different scale
    exact, s0 = D.solve(F, rowptr, col, val, sizes, n_sweeps=64, tol=0.0)
    assert (s0 < 64).all() and (s0 >= 3).all()
    again, s1 = D.solve(exact, rowptr, col, val, sizes, n_sweeps=1)
    assert (s1 == 1).all() and not same_bits(again, exact), "one sweep from f = F is one sweep, whatever F"
    one, s = D.solve(F, rowptr, col, val, sizes, n_sweeps=1, tol=0.0)
    assert (s == 1).all()
    loose, s2 = D.solve(F, rowptr, col, val, sizes, n_sweeps=64, tol=1e-4)
    assert len(set(s2.tolist())) > 1 and (s2 <= s0).all() and s2.min() >= 1, "an absolute tol stops small steps sooner"
    for t in range(12):                                                           # a step's bits are those of n_sweeps = its own count
        assert same_bits(loose[:, t], D.solve(F[:, t:t + 1], rowptr, col, val, sizes, n_sweeps=int(s2[t]), tol=0.0)[0][:, 0])
    capped, s3 = D.solve(F, rowptr, col, val, sizes, n_sweeps=2, tol=0.0)
    assert (s3 == 2).all()
    huge, s4 = D.solve(F, rowptr, col, val, sizes, n_sweeps=64, tol=np.inf)
    assert (s4 == 1).all() and same_bits(huge, one)
    Fn = F.copy()
    Fn[2, 5] = np.nan
    assert D.solve(Fn, rowptr, col, val, sizes, n_sweeps=7, tol=np.inf)[1].tolist() == [1] * 5 + [7] + [1] * 6


# ------------------------------------------------------------------------------------------------ the purpose
@pytest.mark.parametrize("sep", D.SEPARATIONS, ids=lambda s: "sep" + "".join(map(str, s)))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_demixed_traces_follow_their_own_neuron_better(seed, sep):
    """Restatement, bg = 0.05, thr = 0.5, alpha = 0.7.  Recorded over the nine cases: F 0.838 - 0.981 with
    its own amplitude, demixed 0.871 - 0.993; Fc 0.949 - 0.992, demixed 0.982 - 0.999; |correlation| with the partner's amplitude
    0.009 - 0.515 before, 0.000 - 0.288 after; 9 - 17 sweeps to the fixpoint."""
    amp = D.scene(seed, 0.05, sep)[2]
    geo, (w, wsum, sizes), (F, Fnp, Fc), (Fd, sweeps), parts = D.scene_traces(seed, 0.05, sep)
    rF, rFd, rFc, rFdc, xF, xFd = D.purpose(F, Fnp, Fc, Fd, amp)
    P = D.PAIRED
    print(f"seed {seed} sep {sep}: sizes {sizes.tolist()}, sweeps {sweeps.min()} - {sweeps.max()}, M {parts[4].round(3).tolist()}\n"
          f"  F {rF[P].round(3).tolist()} demixed {rFd[P].round(3).tolist()}\n  Fc {rFc[P].round(3).tolist()} demixed {rFdc[P].round(3).tolist()}\n"
          f"  partner: F {xF.round(3).tolist()} demixed {xFd.round(3).tolist()}")
    assert parts[2].tolist() == [0, 1, 2, 3, 4, 5, 6, 6] and parts[3].tolist() == [1, 0, 3, 2, 5, 4], "only partners' boxes meet"
    assert (parts[4] > 0).all() and (sizes > 0).all()
    assert (rFd[P] > rF[P]).all(), "every paired neuron's demixed trace follows its own amplitude strictly better"
    assert (rFdc[P] > rFc[P]).all(), "and so after the neuropil correction"
    assert same_bits(Fd[D.ISOLATED], F[D.ISOLATED]), "the isolated neuron keeps its bits"
    assert sweeps.max() < 64


# ------------------------------------------------------------------------------------------------ the entry points' arguments
BOXES = np.array([[0, 2, 0, 2, 0, 2], [0, 2, 0, 2, 1, 3]], dtype=np.int32)
OFF = np.array([0, 8, 16], dtype=np.int64)
PAIRS = np.array([[0, 0], [0, 1], [1, 1]], dtype=np.int32)
ROWPTR = np.array([0, 1, 2], dtype=np.int32)
COL = np.array([1, 0], dtype=np.int32)


def test_footprint_overlaps_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(3)]                 # w, ws, G

    def call(a=q, boxes=BOXES, off=OFF, N=2, pairs=PAIRS, P=3):
        return L.cwfa_footprint_overlaps_f32(a[0], host(boxes), host(off), N, host(pairs), P, a[1], a[2], None)
    for k in range(3):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_footprint_overlaps_f32: null" in L.cwfa_last_error()
    assert call(boxes=None) == -1 and call(off=None) == -1 and call(pairs=None) == -1
    assert call(N=-1) == -2 and call(P=-1) == -2 and call(P=1 << 31) == -2
    for k in (1, 2):
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert call(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    for b in ([-1, 2, 0, 2, 0, 2], [1, 0, 0, 2, 0, 2], [0, 2, 0, 2, 3, 2]):
        assert call(boxes=np.array([b, BOXES[1]], dtype=np.int32)) == -1 and b"not a box" in L.cwfa_last_error()
    assert call(off=np.array([0, 7, 15], dtype=np.int64)) == -1 and b"offsets" in L.cwfa_last_error()
    assert call(off=np.array([1, 9, 17], dtype=np.int64)) == -1 and b"offsets[0]" in L.cwfa_last_error()
    for bad in ([[0, 0], [0, 2], [1, 1]], [[0, 0], [1, 0], [1, 1]], [[-1, 0], [0, 1], [1, 1]]):
        assert call(pairs=np.array(bad, dtype=np.int32)) == -1 and b"is not 0 <= n <= m" in L.cwfa_last_error()
    for bad in ([[0, 1], [0, 0], [1, 1]], [[0, 0], [0, 0], [1, 1]], [[1, 1], [0, 1], [0, 0]]):
        assert call(pairs=np.array(bad, dtype=np.int32)) == -1 and b"ascend" in L.cwfa_last_error()
    assert call(P=0, pairs=None) == 0 and call(a=[None, None, None], boxes=None, off=np.zeros(1, dtype=np.int64), N=0, pairs=None, P=0) == 0, \
        "no pair: no device work"


def test_demix_plan_arguments(built_lib):
    L = built_lib
    plan = ctypes.c_void_p(123)

    def call(rowptr=ROWPTR, col=COL, N=2, pairs=PAIRS, P=3, out=ctypes.byref(plan)):
        return L.cwfa_demix_plan_create(host(rowptr), host(col), N, host(pairs), P, out)
    i32 = lambda v: np.array(v, dtype=np.int32)
    assert call(out=None) == -1 and call(rowptr=None) == -1 and call(col=None) == -1 and call(pairs=None) == -1
    assert b"cwfa_demix_plan_create: null" in L.cwfa_last_error()
    assert call(N=-1) == -2 and call(P=-1) == -2 and call(P=1 << 31) == -2
    assert call(rowptr=i32([1, 1, 2])) == -1 and b"rowptr[0]" in L.cwfa_last_error()
    assert call(rowptr=i32([0, 2, 1])) == -1 and b"decreases" in L.cwfa_last_error()
    assert call(col=i32([2, 0])) == -1 and call(col=i32([-1, 0])) == -1 and b"is not in 0 .. 1" in L.cwfa_last_error()
    assert call(col=i32([0, 0])) == -1 and b"own diagonal" in L.cwfa_last_error()
    three = dict(rowptr=i32([0, 2, 3, 4]), N=3, pairs=i32([[0, 0], [0, 1], [0, 2], [1, 1], [2, 2]]), P=5)
    assert call(col=i32([2, 1, 0, 0]), **three) == -1 and b"do not ascend" in L.cwfa_last_error()
    assert call(col=i32([1, 1, 0, 0]), **three) == -1 and b"do not ascend" in L.cwfa_last_error()
    assert call(col=i32([1, 2, 2, 0]), **three) == -1 and b"has no pair" in L.cwfa_last_error()
    assert call(pairs=i32([[0, 0], [0, 1]]), P=2) == -1 and b"lacks the diagonal" in L.cwfa_last_error()
    assert call(pairs=i32([[0, 0], [1, 1], [0, 1]])) == -1 and b"ascend" in L.cwfa_last_error()
    assert call(pairs=i32([[0, 0], [0, 2], [1, 1]])) == -1 and b"is not 0 <= n <= m" in L.cwfa_last_error()
    assert plan.value is None, "a refused call leaves no plan behind"
    assert L.cwfa_demix_plan_destroy(None) == -1 and L.cwfa_demix_plan_destroy(ctypes.c_void_p(4096)) == -1
    assert b"not a live plan" in L.cwfa_last_error()


def test_demix_coeffs_and_solve_arguments(built_lib, ptr):
    """Everything that does not need a live plan (which needs a device): the plan is looked at last."""
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(4)]
    bogus = ctypes.c_void_p(ptr.value + 8192)

    def coeffs(a=q, P=3, N=2, plan=bogus):                                        # G, wsum, sizes, val_out
        return L.cwfa_demix_coeffs_f64(plan, a[0], P, a[1], a[2], N, a[3], None)
    for k in range(3):
        args = list(q)
        args[k] = None
        assert coeffs(args) == -1 and b"cwfa_demix_coeffs_f64: null" in L.cwfa_last_error()
    assert coeffs(N=-1) == -2 and coeffs(P=-1) == -2
    for k in (0, 1, 3):
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert coeffs(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    assert coeffs() == -1 and b"not a live plan" in L.cwfa_last_error() and coeffs(plan=None) == -1

    def solve(a=q, fs=4, N=2, T=4, plan=bogus, n_sweeps=8, tol=0.0, nonneg=1):    # F, out, sweeps
        return L.cwfa_demix_solve_f64(a[0], fs, a[1], N, T, plan, n_sweeps, tol, nonneg, a[2], None)
    for k in range(3):
        args = list(q)
        args[k] = None
        assert solve(args) == -1 and b"cwfa_demix_solve_f64: null" in L.cwfa_last_error()
    assert solve([q[0], q[0], q[2]]) == -1 and b"out is F" in L.cwfa_last_error()
    assert solve(N=-1) == -2 and solve(T=-1) == -2
    assert solve(n_sweeps=0) == -1 and solve(n_sweeps=-3) == -1 and b"n_sweeps" in L.cwfa_last_error()
    for tol in (-1e-300, -1.0, float("nan"), -float("inf")):
        assert solve(tol=tol) == -1 and b"tol" in L.cwfa_last_error()
    assert solve(nonneg=2) == -1 and solve(nonneg=-1) == -1
    assert solve(fs=3) == -1 and b"stride" in L.cwfa_last_error()
    for k in (0, 1):
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert solve(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    assert solve() == -1 and b"not a live plan" in L.cwfa_last_error() and solve(plan=None) == -1
    assert solve(tol=float("inf")) == -1 and b"not a live plan" in L.cwfa_last_error(), "an infinite tol is a tol"


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_the_python_layer_refuses_before_any_device_work(built_lib):
    from cwfa_amd import CWFA, _lib, ops
    assert _lib.DEMIX_PAIR_BYTES == 48 and {"demix_plan", "demix_traces"} <= set(CWFA.__all__)
    for bad in (np.zeros((2, 5), dtype=np.int32), np.zeros((2, 6)), "boxes"):
        with pytest.raises(ValueError, match=r"\[N,6\]"):
            ops.footprint_pairs(bad)
    with pytest.raises(ValueError, match="half-open"):
        ops.footprint_pairs([[2, 1, 0, 1, 0, 1]])
    for bad in ([[0, 0], [1, 0]], [[0, 1], [0, 0]], [[0, 0], [0, 2]], [[0, 0], [0, 0]], np.zeros((2, 3), dtype=np.int32), [[0.5, 1.0]]):
        with pytest.raises(ValueError, match="pairs"):
            ops.demix_structure(bad, 2)
    w = torch.zeros(16)
    fp = CWFA.Footprints(BOXES, OFF, w, torch.ones(2, dtype=torch.float64), torch.ones(2, dtype=torch.int32), w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.footprint_overlaps(fp, PAIRS)
    with pytest.raises(ValueError, match="pairs"):
        ops.footprint_overlaps(fp, [[1, 0]])
    with pytest.raises(ValueError, match="NeuronFootprints.finish"):
        ops.footprint_overlaps(object(), PAIRS)
    for bad in (object(), None, (BOXES, OFF)):
        with pytest.raises(ValueError, match="NeuronFootprints.finish"):
            CWFA.demix_plan(bad)
    with pytest.raises(ValueError, match="on the HIP device"):
        CWFA.demix_plan(fp)                                                       # wsum and sizes on the host
    F = torch.zeros(2, 4, dtype=torch.float64)
    for bad in (object(), None, "plan"):
        with pytest.raises(ValueError, match="DemixPlan"):
            CWFA.demix_traces(F, bad)
        with pytest.raises(ValueError, match="DemixPlan"):
            ops.demix_solve(F, bad)
    plan = object.__new__(ops.DemixPlan)                                          # a plan's host side: no device, no handle
    plan.N, plan.handle, plan.device = 2, None, torch.device("cpu")
    for bad in (F.float(), F, F[0], torch.zeros(2, 0, dtype=torch.float64), np.zeros((2, 4)), None):
        with pytest.raises(ValueError, match=r"float64 \[N, T\] tensor on the HIP device"):
            CWFA.demix_traces(bad, plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.demix_solve(F, plan)
    with pytest.raises(ValueError, match="3 rows"):
        CWFA.demix_traces(torch.zeros(3, 4, dtype=torch.float64), plan)
    for bad in (0, -1, 1.5, "many", None):
        with pytest.raises(ValueError, match="n_sweeps"):
            CWFA.demix_traces(F, plan, n_sweeps=bad)
    for bad in (-1e-9, float("nan"), "loose", None):
        with pytest.raises(ValueError, match="tol"):
            CWFA.demix_traces(F, plan, tol=bad)
    for kw in ({"n_sweeps": 0}, {"tol": -1.0}, {"tol": float("nan")}):
        with pytest.raises(ValueError):
            ops.demix_solve(F, plan, **kw)
    assert "delta_f_over_f(Fd, Fnp)" in CWFA.demix_traces.__doc__ and "singular" in CWFA.demix_traces.__doc__

