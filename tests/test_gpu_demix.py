"""GPU: the demixing of overlapping footprints against the numpy restatement tests/demix_ref.py.

The overlap sums use a fixed tree of their own, so they are held to the bound of tests/test_gpu_footprints.py against math.fsum, the
correctly rounded exact sum of the n exact products a_i = w_n(v_i) w_m(v_i): |G_device - fsum| <= n 2^-53 sum |a_i|.  Everything behind
them -- the coefficients, the demixed traces and the sweep counts -- is bit for bit the restatement's given the device's own G."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import demix_ref as D
import footprints_ref as FR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def footprints_of(boxes, seed=0, empty=()):
    """(CWFA.Footprints on the device, host weights, wsum, sizes): weights U(0.5, 1) with three in ten voxels 0, as a thresholded
    correlation looks; the neurons of `empty` have no voxel at all."""
    from cwfa_amd import CWFA
    boxes = np.asarray(boxes, dtype=np.int32).reshape(-1, 6)
    off = FR.offsets_of(boxes)
    rng = np.random.default_rng(seed)
    w = np.where(rng.random(off[-1]) < 0.3, 0.0, rng.uniform(0.5, 1.0, off[-1])).astype(np.float32)
    for n in empty:
        w[off[n]:off[n + 1]] = 0.0
    wsum, sizes = np.zeros(len(boxes)), np.zeros(len(boxes), dtype=np.int32)
    for n in range(len(boxes)):
        total = 0.0
        for v in w[off[n]:off[n + 1]].astype(np.float64).tolist():
            total = total + v
        wsum[n], sizes[n] = total, np.count_nonzero(w[off[n]:off[n + 1]])
    wd = torch.tensor(w).cuda()
    fp = CWFA.Footprints(boxes, off, wd, torch.tensor(wsum).cuda(), torch.tensor(sizes).cuda(), wd)
    return fp, w, wsum, sizes


# ------------------------------------------------------------------------------------------------ overlap sums
def corner_boxes(shape=(5, 9, 11)):
    D_, H, W = shape
    mid = (D_ // 2, H // 2, W // 2)
    centres = [(0, 0, 0), (D_ - 1, H - 1, W - 1), (0, H - 1, W // 2), (D_ - 1, H // 2, 0), (D_ // 2, 0, W - 1), mid, (mid[0], mid[1] + 1, mid[2] + 2)]
    return FR.boxes_of(centres, shape, (2, 3, 3))


def random_boxes(N=130, seed=5, shape=(5, 10, 12), most=(4, 7, 8)):
    rng = np.random.default_rng(seed)
    lo = np.stack([rng.integers(0, n, N) for n in shape], axis=1)
    hi = np.minimum(lo + np.stack([rng.integers(0, m + 1, N) for m in most], axis=1), shape)
    boxes = np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1], lo[:, 2], hi[:, 2]], axis=1).astype(np.int32)
    boxes[(hi <= lo).any(1)] = 0
    return boxes


G_CASES = {
    "1x1x1": [[0, 1, 0, 1, 0, 1], [0, 1, 0, 1, 0, 1], [1, 2, 0, 1, 0, 1], [0, 1, 0, 1, 0, 1]],
    "one_voxel": [[0, 3, 0, 4, 0, 5], [2, 5, 3, 7, 4, 9]],
    "face": [[0, 3, 0, 4, 0, 5], [0, 3, 0, 4, 4, 9], [2, 4, 0, 4, 0, 5]],
    "nested": [[0, 6, 0, 10, 0, 10], [2, 4, 3, 5, 3, 5], [2, 3, 3, 4, 3, 4]],
    "identical": [[1, 4, 2, 7, 3, 9], [1, 4, 2, 7, 3, 9]],
    "clipped": corner_boxes(),
    "empty": [[0, 2, 0, 3, 0, 4], [0, 0, 0, 0, 0, 0], [1, 3, 1, 4, 1, 5], [1, 1, 0, 3, 0, 4]],
    "none": np.zeros((0, 6), dtype=np.int32),
    "one": [[1, 3, 1, 3, 1, 3]],
    "random130": random_boxes(),
}


@pytest.mark.parametrize("name", list(G_CASES))
def test_overlap_sums_within_the_derived_bound_and_repeatable(name):
    from cwfa_amd import ops
    boxes = np.asarray(G_CASES[name], dtype=np.int32).reshape(-1, 6)
    fp, w, wsum, sizes = footprints_of(boxes, seed=3)
    pairs = ops.footprint_pairs(boxes)
    assert np.array_equal(pairs, D.pairs_of(boxes))
    want, mag, terms = D.overlaps(boxes, fp.offsets, w, pairs)
    got = ops.footprint_overlaps(fp, pairs)
    assert got.dtype == torch.float64 and got.shape == (len(pairs),)
    g = got.cpu().numpy()
    err, bound = np.abs(g - want), terms * U * mag
    print(f"{name}: {len(pairs)} pairs, terms up to {terms.max() if len(terms) else 0}, largest error / bound "
          f"{np.max(err / np.maximum(bound, 1e-300)) if len(err) else 0:.3f}")
    assert (err <= bound).all()
    assert not bits(g)[mag == 0].any(), "no term, or only zero products: exactly +0.0"
    assert same_bits(ops.footprint_overlaps(fp, pairs), got), "two runs differ"
    if name == "1x1x1":
        w64 = w.astype(np.float64)
        assert pairs.tolist() == [[0, 0], [0, 1], [0, 3], [1, 1], [1, 3], [2, 2], [3, 3]] and g.tolist() == [
            w64[0] * w64[0], w64[0] * w64[1], w64[0] * w64[3], w64[1] * w64[1], w64[1] * w64[3], w64[2] * w64[2], w64[3] * w64[3]]
    if name == "one_voxel":
        assert terms.tolist() == [60, 1, 60]
    if name == "random130":
        assert len(pairs) > 4 * 130 and (terms == 0).sum() > 0
        far = np.array([[0, 0], [0, 129], [5, 77], [129, 129]], dtype=np.int32)    # pairs whose boxes need not meet: 0.0 where they do not
        sub, smag, _ = D.overlaps(boxes, fp.offsets, w, far)
        gs = ops.footprint_overlaps(fp, far).cpu().numpy()
        assert (np.abs(gs - sub) <= 600 * U * smag).all() and not bits(gs)[smag == 0].any()


def test_overlap_sums_of_weights_past_2_31():
    """The ragged weights of two small overlapping boxes start past 2^31 elements: in front of them two boxes of 1.1e9 voxels each
    whose weights are never touched (allocated, not written, and left out of the pair table).  Against float64 torch on the device."""
    from cwfa_amd import CWFA, ops
    boxes = np.array([[0, 1100, 0, 1000, 0, 1000], [0, 1100, 0, 1000, 0, 1000], [2, 5, 3, 8, 1, 8], [3, 7, 5, 9, 4, 11]], dtype=np.int32)
    off = FR.offsets_of(boxes)
    assert off[2] > 1 << 31
    w = torch.empty(int(off[-1]), device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    w[int(off[2]):] = torch.rand(int(off[-1] - off[2]), device="cuda", generator=gen) + 0.5
    fp = CWFA.Footprints(boxes, off, w, torch.ones(4, dtype=torch.float64).cuda(), torch.ones(4, dtype=torch.int32).cuda(), w)
    pairs = np.array([[2, 2], [2, 3], [3, 3]], dtype=np.int32)
    got = ops.footprint_overlaps(fp, pairs).cpu().numpy()
    a, b = fp.dense(2).double(), fp.dense(3).double()
    ia, ib = a[1:3, 2:5, 3:7], b[0:2, 0:3, 0:4]                                  # the intersection [3,5) x [5,8) x [4,8) in either box
    want = np.array([float((a * a).sum()), float((ia * ib).sum()), float((b * b).sum())])
    mag = np.array([float((a * a).sum()), float((ia * ib).sum()), float((b * b).sum())])
    terms = np.array([a.numel(), ia.numel(), b.numel()])
    assert terms.tolist() == [105, 24, 112] and (np.abs(got - want) <= 2 * terms * U * mag).all(), "both sums are trees: twice the bound"
    assert got[1] > 0
    del w, fp


# ------------------------------------------------------------------------------------------------ coefficients and the solve
def chain_boxes(N=130):
    """Boxes 3 x 4 x 6 every 4 voxels along x: each shares two of its six columns with either neighbour -- one component."""
    return np.array([[0, 3, 0, 4, 4 * k, 4 * k + 6] for k in range(N)], dtype=np.int32)


def pair_boxes(N=40):
    """N separate pairs: two boxes 3 x 4 x 6 that share half their columns, the pairs 6 apart in y."""
    return np.array([[0, 3, 6 * j, 6 * j + 4, 3 * h, 3 * h + 6] for j in range(N) for h in (0, 1)], dtype=np.int32)


def special_boxes():
    """0 and 2 overlap each other and the empty footprint 1 between them; 3 and 4 are a second component; 5 meets nobody."""
    return np.array([[0, 4, 0, 4, 0, 6], [0, 4, 0, 4, 2, 8], [0, 4, 0, 4, 4, 10], [0, 4, 6, 10, 0, 6], [0, 4, 6, 10, 3, 9], [0, 4, 12, 16, 0, 6]],
                    dtype=np.int32)


SYSTEMS = {"chain130": (chain_boxes, ()), "pairs40": (pair_boxes, ()), "special": (special_boxes, (1,))}


@functools.lru_cache(maxsize=None)
def system(name):
    """(footprints, plan, host (pairs, G, rowptr, col, val), sizes): the plan through the library, the restatement's coefficients
    from the device's own G."""
    from cwfa_amd import ops
    make, empty = SYSTEMS[name]
    boxes = make()
    fp, w, wsum, sizes = footprints_of(boxes, seed=len(boxes), empty=empty)
    plan = ops.DemixPlan(fp)
    pairs = D.pairs_of(boxes)
    rowptr, col = D.structure(pairs, len(boxes))
    G = plan.G.cpu().numpy()
    val = D.coefficients(G, pairs, rowptr, col, wsum, sizes)
    return fp, plan, (pairs, G, rowptr, col, val), sizes


@functools.lru_cache(maxsize=None)
def traces_in(N, T, nan=False):
    """float64 [N,T]: values in -0.3 .. 1.7 (the projection has work to do), every time step at a scale of its own between 1e-3 and
    1e3 (an absolute tol stops them at different sweeps); nan: one NaN in row 3 (and 0 at the last step)."""
    rng = np.random.default_rng(1000 * N + T)
    F = (2.0 * rng.random((N, T)) - 0.3) * 10.0 ** rng.uniform(-3, 3, T)[None, :]
    if nan:
        F[3, T // 2] = np.nan
        F[0, T - 1] = np.nan
    F.setflags(write=False)
    return F


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_structure_and_coefficients_are_the_restatement_bit_for_bit(name):
    fp, plan, (pairs, G, rowptr, col, val), sizes = system(name)
    assert np.array_equal(plan.pairs, pairs) and np.array_equal(plan.rowptr, rowptr) and np.array_equal(plan.col, col)
    assert plan.val.dtype == torch.float64 and same_bits(plan.val, val), "coefficients differ"
    M = D.dense_matrix(rowptr, col, val)
    if name == "chain130":
        assert np.diff(rowptr).tolist() == [1] + [2] * 128 + [1] and (val > 0).all() and val.max() < 0.6
    if name == "pairs40":
        assert np.diff(rowptr).tolist() == [1] * 80 and (val > 0).all()
    if name == "special":
        assert np.diff(rowptr).tolist() == [2, 2, 2, 1, 1, 0]
        assert not M[1].any() and not M[:, 1].any() and M[0, 2] > 0 and M[2, 0] > 0, "coupled only through their own G"
        assert G[list(map(tuple, pairs.tolist())).index((1, 1))] == 0.0


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_traces_and_sweeps_are_the_restatement_bit_for_bit(name, T):
    """nonneg on and off, tol = 0 and a tol that stops time steps at different sweeps, n_sweeps = 1, a sweep limit that cuts the
    iteration short, and a row-strided view of F."""
    from cwfa_amd import ops
    fp, plan, (pairs, G, rowptr, col, val), sizes = system(name)
    N = len(sizes)
    F = traces_in(N, T)
    Fd = torch.tensor(F).cuda()
    wide = torch.full((N, T + 5), -7.0, dtype=torch.float64, device="cuda")
    wide[:, :T] = Fd
    view = wide[:, :T]
    assert view.stride(0) == T + 5
    counts = {}
    for n_sweeps, tol, nonneg in ((64, 0.0, True), (64, 0.0, False), (64, 1e-6, True), (1, 0.0, True), (3, 0.0, False)):
        want, ws = D.solve(F, rowptr, col, val, sizes, n_sweeps, tol, nonneg)
        got, gs = ops.demix_solve(view if nonneg else Fd, plan, n_sweeps, tol, nonneg)
        assert got.shape == (N, T) and gs.dtype == torch.int32 and gs.shape == (T,)
        assert np.array_equal(gs.cpu().numpy(), ws), f"sweeps differ at {(n_sweeps, tol, nonneg)}"
        assert same_bits(got, want), f"traces differ at {(n_sweeps, tol, nonneg)}"
        counts[(n_sweeps, tol)] = ws
    assert (wide[:, T:] == -7.0).all() and same_bits(wide[:, :T], F), "F is only read"
    assert (counts[(1, 0.0)] == 1).all() and (counts[(3, 0.0)] <= 3).all()
    assert (counts[(64, 0.0)] < 64).all() and (counts[(64, 1e-6)] <= counts[(64, 0.0)]).all()
    if T >= 63:
        assert len(set(counts[(64, 1e-6)].tolist())) > 1, "the tol stops different time steps at different sweeps"
    if name == "special":
        got = ops.demix_solve(Fd, plan)[0]
        assert torch.isnan(got[1]).all() and same_bits(got[5], np.where(F[5] < 0, 0.0, F[5])) and not torch.isnan(got[[0, 2, 3, 4, 5]]).any()
        assert same_bits(ops.demix_solve(Fd, plan, nonneg=False)[0][5], F[5]), "a neuron that meets nobody returns the bits of its F"


def test_special_values_and_chunks_on_the_device():
    """A NaN in F stays inside its component and its time step, which runs to the sweep limit; T cut in chunks equals T whole."""
    from cwfa_amd import ops
    fp, plan, (pairs, G, rowptr, col, val), sizes = system("special")
    T = 257
    clean, F = traces_in(6, T), traces_in(6, T, nan=True)
    Fd = torch.tensor(F).cuda()
    for nonneg in (True, False):
        want, ws = D.solve(F, rowptr, col, val, sizes, 20, 0.0, nonneg)
        got, gs = ops.demix_solve(Fd, plan, 20, 0.0, nonneg)
        assert same_bits(got, want) and np.array_equal(gs.cpu().numpy(), ws)
        base, bs = D.solve(clean, rowptr, col, val, sizes, 20, 0.0, nonneg)
        g = got.cpu().numpy()
        assert np.isnan(g[3:5, T // 2]).all() and np.isnan(g[[0, 2], T - 1]).all() and ws[T // 2] == 20 and ws[T - 1] == 20
        hit = np.zeros((6, T), dtype=bool)
        hit[3:5, T // 2] = hit[[0, 2], T - 1] = hit[1, :] = True
        assert not np.isnan(g[~hit]).any() and np.array_equal(bits(g)[~hit], bits(base)[~hit]), "nobody else sees the NaN"
        parts, t = [], 0
        for n in (1, 63, 64, 65, 64):
            parts.append(ops.demix_solve(Fd[:, t:t + n], plan, 20, 0.0, nonneg))
            t += n
        assert t == T and same_bits(torch.cat([p[0] for p in parts], dim=1), got) and torch.equal(torch.cat([p[1] for p in parts]), gs)


def test_no_neuron_one_neuron_and_a_mismatched_plan():
    from cwfa_amd import CWFA, _lib, ops
    fp0 = footprints_of(np.zeros((0, 6), dtype=np.int32))[0]
    plan0 = CWFA.demix_plan(fp0)
    assert plan0.N == 0 and plan0.E == 0 and plan0.G.shape == (0,)
    Fd, sweeps = CWFA.demix_traces(torch.zeros(0, 5, dtype=torch.float64, device="cuda"), plan0)
    assert Fd.shape == (0, 5) and sweeps.tolist() == [1] * 5
    fp1 = footprints_of([[1, 3, 1, 3, 1, 3]])[0]
    F = torch.tensor(traces_in(1, 65)).cuda()
    for arg in (fp1, CWFA.demix_plan(fp1)):
        Fd, sweeps = CWFA.demix_traces(F, arg, nonneg=False)
        assert same_bits(Fd, F) and (sweeps == 1).all()
    fp, plan, _, sizes = system("special")
    with pytest.raises(ValueError, match="1 rows"):
        CWFA.demix_traces(F, plan)
    L = _lib.lib()
    out, sw = torch.full((1, 65), -7.0, dtype=torch.float64, device="cuda"), torch.zeros(65, dtype=torch.int32, device="cuda")
    rc = L.cwfa_demix_solve_f64(F.data_ptr(), 65, out.data_ptr(), 1, 65, plan.handle, 4, 0.0, 1, sw.data_ptr(), None)
    assert rc == -2 and b"the plan has 6 neurons" in L.cwfa_last_error()
    rc = L.cwfa_demix_coeffs_f64(plan.handle, plan.G.data_ptr(), len(plan.pairs) - 1, fp.wsum.data_ptr(), fp.sizes.data_ptr(), 6, None, None)
    assert rc == -2 and b"the plan has N = 6" in L.cwfa_last_error()
    gone = ops.DemixPlan(fp1)
    handle = ctypes.c_void_p(gone.handle.value)
    del gone
    rc = L.cwfa_demix_solve_f64(F.data_ptr(), 65, out.data_ptr(), 1, 65, handle, 4, 0.0, 1, sw.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1 and b"not a live plan" in L.cwfa_last_error() and (out == -7.0).all(), "refused before any launch"


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("case", [(0, D.SEPARATIONS[0]), (1, D.SEPARATIONS[1]), (2, D.SEPARATIONS[2])], ids=["seed0_005", "seed1_034", "seed2_104"])
def test_scene_to_demixed_traces(case):
    """scene -> ActivityMap(neighbours=26) -> find_neurons(kind="corr", thr=0.9, dist=(2, 3, 3)) -> NeuronFootprints -> finish(0.5) ->
    extract_traces -> demix_traces, all in chunks of 8.  The detector separates the partners at every separation (dist is below
    each); thr = 0.9 keeps the seven planted neurons (scores above 0.97) and drops the maxima of the common background (up to 0.86
    at this dist).  Coefficients, demixed traces and sweeps are bitwise the restatement's given the device's own G and F; every
    paired neuron's demixed trace follows its planted amplitude strictly better than its raw trace, before and after the neuropil
    correction, and the isolated neuron keeps its bits."""
    from cwfa_amd import CWFA
    seed, sep = case
    xh, centres, amp = D.scene(seed, 0.05, sep)
    xd = torch.tensor(xh).cuda()
    T = xh.shape[0]
    am = CWFA.ActivityMap(D.SHAPE, "cuda", neighbours=26)
    for t in range(0, T, 8):
        am.update(xd[t:t + 8])
    coords, scores = CWFA.find_neurons(am, kind="corr", thr=0.9, dist=(2, 3, 3))
    shift = D.SHAPE[0] // 2 + (-25 // 2)
    found = np.array([[z + shift, y, x] for x, y, z in coords])
    near = (np.abs(found[:, None, :] - centres[None, :, :]) <= 1).all(-1)
    assert len(coords) == 7 and near.any(0).all(), "every planted neuron is found within a voxel, partners apart"
    match = near.argmax(0)
    nf = CWFA.NeuronFootprints(coords, D.SHAPE, "cuda")
    for t in range(0, T, 8):
        nf.update(xd[t:t + 8])
    fp = nf.finish(0.5)
    plan = CWFA.demix_plan(fp)
    parts = [CWFA.extract_traces(xd[t:t + 8], fp, nf.geometry, alpha=0.7) for t in range(0, T, 8)]
    demixed = [CWFA.demix_traces(p[0], plan) for p in parts]
    Ft, Fnp, Fc = (torch.cat([p[k] for p in parts], dim=1) for k in range(3))
    Fd, sweeps = torch.cat([d[0] for d in demixed], dim=1), torch.cat([d[1] for d in demixed])
    whole = CWFA.demix_traces(Ft, fp)
    assert same_bits(whole[0], Fd) and torch.equal(whole[1], sweeps), "chunks of 8 against the whole series, the plan made on the way"
    Ft, Fnp, Fc, Fd = (t.cpu().numpy() for t in (Ft, Fnp, Fc, Fd))
    w, wsum, sizes = fp.weights.cpu().numpy(), fp.wsum.cpu().numpy(), fp.sizes.cpu().numpy()
    want, ws, (pairs, G, rowptr, col, val) = D.demix(Ft, fp.boxes, fp.offsets, w, wsum, sizes, G=plan.G.cpu().numpy())
    ref_G, mag, terms = D.overlaps(fp.boxes, fp.offsets, w, pairs)
    assert np.array_equal(plan.pairs, pairs) and (np.abs(G - ref_G) <= terms * U * mag).all()
    assert same_bits(plan.val, val) and same_bits(Fd, want) and np.array_equal(sweeps.cpu().numpy(), ws)
    partner = {int(match[n]): int(match[n ^ 1]) for n in D.PAIRED}
    assert all(col[rowptr[n]:rowptr[n + 1]].tolist() == [m] for n, m in partner.items()) and rowptr[match[6] + 1] == rowptr[match[6]]
    rF, rFd, rFc, rFdc, xF, xFd = D.purpose(Ft[match], Fnp[match], Fc[match], Fd[match], amp)
    P = D.PAIRED
    print(f"seed {seed} sep {sep}: sizes {sizes[match].tolist()}, sweeps {ws.min()} - {ws.max()}, M {val.round(3).tolist()}\n"
          f"  F {rF[P].round(3).tolist()} demixed {rFd[P].round(3).tolist()}\n  Fc {rFc[P].round(3).tolist()} demixed {rFdc[P].round(3).tolist()}\n"
          f"  partner: F {xF.round(3).tolist()} demixed {xFd.round(3).tolist()}")
    assert (rFd[P] > rF[P]).all() and (rFdc[P] > rFc[P]).all()
    assert same_bits(Fd[match[6]], Ft[match[6]]), "the isolated neuron keeps its bits"
