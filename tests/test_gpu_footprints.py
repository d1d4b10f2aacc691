"""GPU: the neuron footprints against the numpy restatement tests/footprints_ref.py.

Bit for bit: the state of cwfa_footprint_update_f32 for every chunking and the smallest shapes at which the kernel can go wrong, the
correlation, the selection (weights, sizes, wsum), the occupancy map.  The traces' reductions use a fixed tree of their own, so they
are held to a derived bound against math.fsum, the correctly rounded exact sum S of the n exact products a_i = w_i x_i: a tree adds
with at most n - 1 roundings on any path, each at most 2^-53 relative to a partial sum of magnitude at most M = sum |a_i|, and fsum
rounds once:
    |sum_device - fsum| <= n 2^-53 M.
A trace divides the sum by wsum (one more rounding on either side): (n + 2) 2^-53 M / wsum; Fc = fl(F - fl(alpha Fnp)) adds the two
bounds (the second times alpha) and one rounding of the product and of the difference on either side."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import footprints_ref as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 4), (2, 3, 8), (6, 36, 44), (7, 37, 45)]
CHUNKS = [(1,) * 7, (3, 4), (7,), (1, 2, 4), "strided"]
U = 2.0 ** -53
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def stack(shape, T=7):
    """(host, device) [T, *shape]: a mean of 100, a spread of 1, and a component shared by all voxels."""
    rng = np.random.default_rng(11)
    common = rng.standard_normal((T, 1, 1, 1))
    x = (100.0 + 0.7 * common + rng.standard_normal((T, *shape))).astype(np.float32)
    x.setflags(write=False)
    return x, torch.tensor(x).cuda()


@functools.lru_cache(maxsize=None)
def geometry(shape, many=False, whole=True):
    """(restatement's, the library's): the whole volume as one box (whole: it occupies every shell), boxes clipped at every face and
    corner, two overlapping boxes in the middle and an empty one; many: 130 random boxes instead (more than two argument chunks), some
    of them empty."""
    from cwfa_amd import ops
    D, H, W = shape
    if many:
        rng = np.random.default_rng(5)
        lo = np.stack([rng.integers(0, n, 130) for n in shape], axis=1)
        hi = np.minimum(lo + np.stack([rng.integers(0, m + 1, 130) for m in (3, 4, 5)], axis=1), shape)
        boxes = np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1], lo[:, 2], hi[:, 2]], axis=1).astype(np.int32)
        boxes[(hi <= lo).any(1)] = 0
    else:
        mid = (D // 2, H // 2, W // 2)
        centres = [(0, 0, 0), (D - 1, H - 1, W - 1), (0, H - 1, W // 2), (D - 1, H // 2, 0), (D // 2, 0, W - 1), mid, (mid[0], mid[1] + 1, mid[2] + 2)]
        boxes = np.concatenate([[[0, D, 0, H, 0, W]] if whole else np.zeros((0, 6)), F.boxes_of(centres, shape, (2, 3, 3)),
                                np.zeros((1, 6))]).astype(np.int32)
    cores = boxes.copy()
    cores[:, 1::2] = np.minimum(cores[:, 0::2] + 1, cores[:, 1::2])             # the box's first voxel (empty for an empty box)
    ref = F.Geometry(None, shape, boxes=boxes, cores=cores, gap=(0, 1, 1), annulus=(1, 2, 2))
    mine = ops.footprint_geometry(boxes, cores, shape, (0, 1, 1), (1, 2, 2), "cuda")
    assert np.array_equal(mine.offsets, ref.offsets) and np.array_equal(mine.shell_outer, ref.outer) and np.array_equal(mine.shell_inner, ref.inner)
    return ref, mine


@functools.lru_cache(maxsize=None)
def traces_in(N, T=7):
    """Reference traces made in numpy: (c, u) float64 [N,T] on the host and on the device."""
    rng = np.random.default_rng(N)
    c, u = 50.0 + rng.standard_normal((N, T)), 10.0 + 3.0 * rng.standard_normal((N, T))
    return c, u, torch.tensor(c).cuda(), torch.tensor(u).cuda()


@functools.lru_cache(maxsize=None)
def reference(shape, with_u, many=False):
    ref = geometry(shape, many)[0]
    c, u = traces_in(ref.N)[:2]
    state = F.accumulate(stack(shape)[0], ref, c, u if with_u else None)
    return state, F.correlate(state[1], state[2], ref, 7, with_u)


def within(got, want, bound):
    """Elementwise: both NaN, or no further apart than the bound."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(want), np.isnan(got), np.abs(got - want) <= bound)


def cuts(x, chunks):
    """[(view, t0, t1)]: the chunkings of section 22; "strided": 3 + 4 of a view whose time stride exceeds a volume."""
    if chunks == "strided":
        T, m = x.shape[0], x[0].numel()
        wide = torch.zeros(T, m + 8, device="cuda")
        wide[:, :m] = x.reshape(T, m)
        view = wide.as_strided(tuple(x.shape), (m + 8, x.shape[2] * x.shape[3], x.shape[3], 1))
        assert view.stride(0) == m + 8 and torch.equal(view, x)
        x, chunks = view, (3, 4)
    out, t = [], 0
    for n in chunks:
        out.append((x[t:t + n], t, t + n))
        t += n
    assert t == x.shape[0]
    return out


def device_state(shape, chunks, with_u, many=False):
    from cwfa_amd import ops
    ref, mine = geometry(shape, many)
    cd, ud = traces_in(ref.N)[2:]
    state = ops.footprint_state(mine, "cuda")
    for k, t in enumerate(state):
        t.view(torch.uint8).fill_(0xA5 if k == 0 else 0x7F)                   # the first chunk writes every element: no stale value survives
    for view, t0, t1 in cuts(stack(shape)[1], chunks):
        ops.footprint_update(view, mine, cd[:, t0:t1], ud[:, t0:t1] if with_u else None, state, first=t0 == 0)
    return state


# ------------------------------------------------------------------------------------------------ the state and the correlation
@pytest.mark.parametrize("with_u", [True, False], ids=["u", "no_u"])
@pytest.mark.parametrize("chunks", CHUNKS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_state_and_correlation_are_the_restatement_bit_for_bit(shape, chunks, with_u):
    from cwfa_amd import ops
    (x0, acc, ref7), corr = reference(shape, with_u)
    state = device_state(shape, chunks, with_u)
    assert same_bits(state[0], x0), "x0 differs"
    assert same_bits(state[2], ref7), "the per-neuron sums differ"
    assert same_bits(state[1], acc), "s1 / s2 / sc / su differ"
    got = ops.footprint_corr(state, geometry(shape)[1], 7, with_u)
    assert same_bits(got, corr) and not torch.isnan(got).any()


@pytest.mark.parametrize("with_u", [True, False], ids=["u", "no_u"])
@pytest.mark.parametrize("chunks", [(7,), (1, 2, 4)], ids=ids)
def test_130_boxes_pass_the_argument_chunks(chunks, with_u):
    from cwfa_amd import ops
    shape = (3, 5, 4)
    (x0, acc, ref7), corr = reference(shape, with_u, True)
    state = device_state(shape, chunks, with_u, True)
    assert same_bits(state[0], x0) and same_bits(state[1], acc) and same_bits(state[2], ref7)
    assert same_bits(ops.footprint_corr(state, geometry(shape, True)[1], 7, with_u), corr)


def test_no_neuron_at_all():
    from cwfa_amd import ops
    x = stack((3, 5, 4))[1]
    g = ops.footprint_geometry(np.zeros((0, 6), dtype=np.int32), np.zeros((0, 6), dtype=np.int32), (3, 5, 4), device="cuda")
    state = ops.footprint_state(g, "cuda")
    none = torch.zeros(0, 7, dtype=torch.float64, device="cuda")
    ops.footprint_update(x, g, none, none, state, True)
    assert ops.footprint_corr(state, g, 7).shape == (0,)
    w, wsum, sizes = ops.footprint_select(torch.zeros(0, device="cuda"), g, 0.5)
    assert w.shape == (0,) and wsum.shape == (0,) and sizes.shape == (0,)
    assert ops.roi_weighted_sums(x, g.boxes).shape == (0, 7) and ops.roi_shell_sums(x, g)[0].shape == (0, 7)
    assert not ops.roi_mark(g.boxes, (3, 5, 4)).any()


@pytest.mark.parametrize("neuropil", [True, False], ids=["u", "no_u"])
def test_special_values_on_the_device(neuropil):
    """A constant voxel, NaN, +inf, -inf (also as a first sample): corr is 0 at exactly those voxels and the restatement's bits at the
    others; NaN or inf in a reference trace; one sample."""
    from cwfa_amd import ops
    x, ref, c, u, planted = F.special_case()
    clean = F.small_case(T=6, seed=4)[0]
    boxes_cores = (ref.boxes, ref.cores)
    mine = ops.footprint_geometry(*boxes_cores, ref.shape, device="cuda")

    def device(xs, cs, us, T=6):
        state = ops.footprint_state(mine, "cuda")
        ops.footprint_update(torch.tensor(xs[:T]).cuda(), mine, torch.tensor(cs[:, :T]).cuda(), None if us is None else torch.tensor(us[:, :T]).cuda(),
                             state, True)
        want = F.accumulate(xs[:T], ref, cs[:, :T], None if us is None else us[:, :T])
        assert all(same_bits(a, b) for a, b in zip(state, want)), "the state with special values differs"
        got = ops.footprint_corr(state, mine, T, neuropil)
        assert same_bits(got, F.correlate(want[1], want[2], ref, T, neuropil)) and not torch.isnan(got).any()
        return got.cpu().numpy()
    uu = u if neuropil else None
    base, got = device(clean, c, uu), device(x, c, uu)
    rest = np.setdiff1d(np.arange(ref.V), planted)
    assert not got[planted].any() and base[planted].all() and np.array_equal(got[rest].view(np.uint32), base[rest].view(np.uint32))
    for bad in (np.nan, np.inf, -np.inf):
        cb = c.copy()
        cb[0, 2] = bad
        assert not device(clean, cb, uu).any()
    assert not device(clean, c, uu, T=1).any()
    if neuropil:
        ub = u.copy()
        ub[0, 3] = np.nan
        plain = F.correlate(*F.accumulate(clean, ref, c, None)[1:], ref, 6, False)
        assert np.array_equal(device(clean, c, ub).view(np.uint32), plain.view(np.uint32))


# ------------------------------------------------------------------------------------------------ selection
def run_select(ref, corr, thr=0.5):
    from cwfa_amd import ops
    mine = ops.footprint_geometry(ref.boxes, ref.cores, ref.shape, device="cuda")
    got = ops.footprint_select(torch.tensor(corr).cuda(), mine, thr)
    want = F.select(corr, ref, thr)
    assert same_bits(got[0], want[0]), "weights differ"
    assert same_bits(got[2], want[2]), "sizes differ"
    assert same_bits(got[1], want[1]), "wsum differs"
    return got, want


@pytest.mark.parametrize("name", ["island", "diagonal", "core_below", "serpentine"])
def test_fill_on_hand_made_maps(name):
    above, core, expect = F.fill_case(name)
    ref, corr = F.box_case(above, core)
    rng = np.random.default_rng(1)
    corr = np.where(above, rng.uniform(0.5, 1.0, corr.shape).astype(np.float32).reshape(above.shape), np.float32(0.25)).ravel().astype(np.float32)
    got, want = run_select(ref, corr)
    assert np.array_equal(F.dense(got[0].cpu().numpy(), ref, 0) != 0, expect) and int(got[2][0]) == expect.sum()


def test_a_box_filled_completely_and_a_threshold_equal_to_a_value():
    dims = (6, 10, 10)
    ref, corr = F.box_case(np.ones(dims, dtype=bool), [2, 5, 4, 7, 2, 4], value=0.5)
    got, want = run_select(ref, corr, 0.5)
    assert int(got[2][0]) == 600 and float(got[1][0]) == 300.0, "corr == thr is above"
    below = np.nextafter(np.float32(0.5), np.float32(0))
    corr2 = corr.copy().reshape(dims)
    corr2[:, :, 5] = below                                                        # a wall one ulp below: the far half is cut off
    got, want = run_select(ref, corr2.ravel(), 0.5)
    assert int(got[2][0]) == 6 * 10 * 5 and not F.dense(got[0].cpu().numpy(), ref, 0)[:, :, 5:].any()
    got, want = run_select(ref, corr2.ravel(), float(below))
    assert int(got[2][0]) == 600


def test_random_maps_in_130_boxes_and_two_runs():
    from cwfa_amd import ops
    rng = np.random.default_rng(8)
    sizes = np.stack([rng.integers(0, m + 1, 130) for m in (6, 10, 10)], axis=1)
    sizes[(sizes == 0).any(1)] = 0
    boxes = np.stack([0 * sizes[:, 0], sizes[:, 0], 0 * sizes[:, 1], sizes[:, 1], 0 * sizes[:, 2], sizes[:, 2]], axis=1).astype(np.int32)
    centres = sizes // 2
    ref = F.Geometry(centres, (6, 10, 10), boxes=boxes)
    corr = rng.uniform(0.0, 1.0, ref.V).astype(np.float32)
    corr[rng.integers(0, ref.V, 50)] = np.nan                                     # NaN is not above
    for thr in (0.3, 0.5):
        got, want = run_select(ref, corr, thr)
        again = run_select(ref, corr, thr)[0]
        assert all(same_bits(a, b) for a, b in zip(got, again)), "two runs differ"
    assert 0 < int(want[2].max()) < 600 and (want[2] == 0).any()


def test_the_largest_box_and_one_voxel_more():
    from cwfa_amd import _lib, ops
    dims = (32, 32, 32)
    rng = np.random.default_rng(2)
    above = rng.uniform(0, 1, dims) < 0.6
    above[15:18, 15:18, 15:18] = True
    ref, corr = F.box_case(above, [15, 18, 15, 18, 15, 18])
    got, want = run_select(ref, corr)
    assert ref.V == 1 << 15 and 1000 < int(got[2][0]) < (1 << 15)
    dims = (9, 11, 331)
    assert dims[0] * dims[1] * dims[2] == (1 << 15) + 1
    big, corr = F.box_case(np.ones(dims, dtype=bool), [0, 1, 0, 1, 0, 1])
    g = ops.footprint_geometry(big.boxes, big.cores, dims, device="cuda")
    with pytest.raises(ValueError, match="more than 32768 voxels"):
        ops.footprint_select(torch.tensor(corr).cuda(), g, 0.5)
    c, w = torch.tensor(corr).cuda(), torch.zeros(big.V, device="cuda")
    ws, sz = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    h = lambda a: ctypes.c_void_p(a.ctypes.data)
    L = _lib.lib()
    rc = L.cwfa_footprint_select_f32(c.data_ptr(), h(g.boxes), h(g.cores), h(g.offsets), 1, 0.5, w.data_ptr(), ws.data_ptr(), sz.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -2 and b"2^15" in L.cwfa_last_error() and not w.any(), "refused before any launch"


# ------------------------------------------------------------------------------------------------ occupancy, box sums, shell sums
@pytest.mark.parametrize("case", [((1, 1, 1), False), ((7, 37, 45), False), ((3, 5, 4), True)], ids=["1x1x1", "7x37x45", "130"])
def test_roi_mark_is_exact(case):
    from cwfa_amd import ops
    ref, mine = geometry(*case)
    occ = ops.roi_mark(ref.boxes, ref.shape)
    assert occ.dtype == torch.uint8 and np.array_equal(occ.cpu().numpy(), ref.occ)
    assert np.array_equal(mine.occupancy.cpu().numpy(), ref.occ)


@pytest.mark.parametrize("case", [((1, 1, 1), False), ((3, 5, 4), False), ((7, 37, 45), False), ((3, 5, 4), True)], ids=["1x1x1", "3x5x4", "7x37x45", "130"])
def test_weighted_sums_within_the_derived_bound(case):
    from cwfa_amd import ops
    ref, mine = geometry(*case)
    xh, xd = stack(case[0])
    w = np.random.default_rng(3).uniform(-1.0, 1.0, ref.V).astype(np.float32)
    for weights in (None, w):
        want, mag, terms = F.weighted_sums(xh, ref.boxes, ref.offsets, weights)
        got = ops.roi_weighted_sums(xd, ref.boxes, None if weights is None else torch.tensor(weights).cuda(), ref.offsets).cpu().numpy()
        err, bound = np.abs(got - want), terms[:, None] * U * mag
        print(f"{case}: weights {weights is not None}: largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert got.shape == want.shape and (err <= bound).all()
        assert not got[terms == 0].any(), "an empty box sums to 0"
    plain, mag, terms = F.weighted_sums(xh, ref.boxes, ref.offsets)
    got = ops.roi_weighted_sums(xd, ref.boxes).cpu().numpy()
    means = ops.roi_means(xd, ref.boxes).cpu().numpy()
    live = terms > 0
    tol = (2 * terms[live, None] + 2) * U * mag[live] / terms[live, None]          # two sums within the bound, two divisions
    assert (np.abs(got[live] / terms[live, None] - means[live]) <= tol).all() and np.isnan(means[~live]).all()
    strided = cuts(xd, "strided")[0][0]
    assert same_bits(ops.roi_weighted_sums(strided, ref.boxes), got[:, :3]), "a time stride above a volume"


@pytest.mark.parametrize("case", [((1, 1, 1), False), ((3, 5, 4), False), ((6, 36, 44), False), ((7, 37, 45), False), ((3, 5, 4), True)],
                         ids=["1x1x1", "3x5x4", "6x36x44", "7x37x45", "130"])
def test_shell_sums_within_the_derived_bound_and_counts_exact(case):
    from cwfa_amd import ops
    ref, mine = geometry(*case, whole=False)
    xh, xd = stack(case[0])
    want, mag, counts = F.shell_sums(xh, ref)
    sums, cnt = ops.roi_shell_sums(xd, mine)
    assert cnt.dtype == torch.int32 and np.array_equal(cnt.cpu().numpy(), counts), "counts differ"
    err, bound = np.abs(sums.cpu().numpy() - want), counts[:, None] * U * mag
    assert (err <= bound).all()
    if not case[1] and min(case[0]) >= 6:                                         # the small volumes are all box
        assert counts[:-1].min() > 0 and counts[-1] == 0, "shells clipped by the volume hold voxels; the empty box's holds none"
    assert same_bits(ops.roi_shell_sums(cuts(xd, "strided")[0][0], mine)[0], sums[:, :3])


def test_a_fully_occupied_shell_gives_nan_and_leaves_the_trace_uncorrected():
    from cwfa_amd import CWFA, ops
    shape = (6, 36, 44)
    ref, mine = geometry(shape)                                                   # its first box is the whole volume: every shell is occupied
    xh, xd = stack(shape)
    sums, cnt = ops.roi_shell_sums(xd, mine)
    assert not cnt.any() and not sums.any()
    w = torch.tensor(np.random.default_rng(4).uniform(0.5, 1.0, ref.V).astype(np.float32)).cuda()
    wsum = torch.tensor([float(w[int(a):int(b)].double().sum()) for a, b in zip(ref.offsets[:-1], ref.offsets[1:])], dtype=torch.float64).cuda()
    fp = CWFA.Footprints(mine.boxes, mine.offsets, w, wsum, torch.zeros(ref.N, dtype=torch.int32).cuda(), w)
    Ft, Fnp, Fc = CWFA.extract_traces(xd, fp, mine)
    assert torch.isnan(Fnp).all() and same_bits(Fc, Ft) and torch.isnan(Ft[-1]).all() and not torch.isnan(Ft[:-1]).any()
    F2, Fnp2, Fc2 = CWFA.extract_traces(xd, fp)
    assert same_bits(F2, Ft) and torch.isnan(Fnp2).all() and same_bits(Fc2, Ft)


# ------------------------------------------------------------------------------------------------ linear offsets past 2^31
def test_offsets_past_2_31():
    """A 2 x 32768 x 34000 volume (2.2e9 voxels), one box at the origin and one at the far corner, T = 2 as 1 + 1, against float64 torch
    on the device: with one step after the first, every sum is its single term."""
    from cwfa_amd import ops
    shape = (2, 32768, 34000)
    boxes = np.array([[0, 2, 0, 3, 0, 5], [1, 2, 32764, 32768, 33993, 34000]], dtype=np.int32)
    cores = np.array([[0, 1, 0, 1, 0, 1], [1, 2, 32767, 32768, 33999, 34000]], dtype=np.int32)
    g = ops.footprint_geometry(boxes, cores, shape, device="cuda")
    x = torch.empty(2, *shape, device="cuda")
    assert x[0].numel() > 1 << 31
    gen = torch.Generator(device="cuda").manual_seed(0)
    for b in boxes:
        r = F.region(b)
        x[(slice(None), *r)] = 100.0 + torch.randn(2, *x[0][r].shape, device="cuda", generator=gen)
    c = ops.roi_weighted_sums(x, cores)
    assert torch.equal(c, torch.stack([x[(slice(None), *F.region(b))].double().reshape(2, -1).sum(1) for b in cores]))
    u = torch.tensor([[3.0, 4.5], [-1.0, 2.25]], dtype=torch.float64, device="cuda")
    state = ops.footprint_state(g, "cuda")
    ops.footprint_update(x[0:1], g, c[:, 0:1], u[:, 0:1], state, True)
    ops.footprint_update(x[1:2], g, c[:, 1:2], u[:, 1:2], state, False)
    for n, b in enumerate(boxes):
        lo, hi = int(g.offsets[n]), int(g.offsets[n + 1])
        v = x[(slice(None), *F.region(b))].reshape(2, -1)
        d = v[1].double() - v[0].double()
        e, gg = c[n, 1] - c[n, 0], u[n, 1] - u[n, 0]
        assert torch.equal(state[0][lo:hi], v[0])
        assert torch.equal(state[1][:, lo:hi], torch.stack([d, d * d, d * e, d * gg]))
        assert torch.equal(state[2][n], torch.stack([c[n, 0], u[n, 0], e, e * e, gg, gg * gg, e * gg]))
    del x


# ------------------------------------------------------------------------------------------------ the class, and end to end
def test_the_class_takes_single_volumes_and_any_chunking():
    from cwfa_amd import CWFA, ops
    shape = (6, 36, 44)
    xh, xd = stack(shape)
    shift = shape[0] // 2 + (-25 // 2)
    centres = [(3, 18, 22), (2, 20, 27), (0, 0, 0), (5, 35, 43)]
    coords = [[x, y, z - shift] for z, y, x in centres]
    ref = F.Geometry(centres, shape)
    runs = []
    for chunks in ((7,), (0,) * 7, (3, 4), (1, 2, 4)):
        nf = CWFA.NeuronFootprints(coords, shape, "cuda")
        t = 0
        for n in chunks:
            nf.update(xd[t] if n == 0 else xd[t:t + n])
            t += max(n, 1)
        assert nf.count == 7
        runs.append(nf)
    g = runs[0].geometry
    assert np.array_equal(g.boxes, ref.boxes) and np.array_equal(g.cores, ref.cores)
    c, u = ops.roi_weighted_sums(xd, g.cores).cpu().numpy(), ops.roi_shell_sums(xd, g)[0].cpu().numpy()
    want = F.accumulate(xh, ref, c, u)
    for nf in runs:
        assert all(same_bits(a, b) for a, b in zip(nf.state, want))
    fp = runs[1].finish(0.3)
    corr = F.correlate(want[1], want[2], ref, 7, True)
    w, wsum, sizes = F.select(corr, ref, 0.3)
    assert same_bits(fp.corr, corr) and same_bits(fp.weights, w) and same_bits(fp.wsum, wsum) and same_bits(fp.sizes, sizes)
    assert fp.dense(1).shape == (5, 10, 10) and same_bits(fp.dense(1), F.dense(w, ref, 1))
    runs[1].update(xd[:2])
    assert runs[1].count == 9, "the state is kept: more volumes may follow"


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scene_to_traces(seed):
    """scene -> ActivityMap(neighbours=26) -> find_neurons(kind="corr") -> NeuronFootprints -> finish -> extract_traces, all in chunks of
    8: footprints equal the restatement's given the device's own reference traces, the traces are within the derived bound, and
    the corrected trace of every planted neuron follows its amplitude better than the box mean does, and above 0.9."""
    from cwfa_amd import CWFA, ops
    xh, centres, amp = F.scene(seed, 0.05)
    xd = torch.tensor(xh).cuda()
    T = xh.shape[0]
    am = CWFA.ActivityMap(F.SHAPE, "cuda", neighbours=26)
    for t in range(0, T, 8):
        am.update(xd[t:t + 8])
    coords, scores = CWFA.find_neurons(am, kind="corr", thr=0.5)
    shift = F.SHAPE[0] // 2 + (-25 // 2)
    found = np.array([[z + shift, y, x] for x, y, z in coords])
    near = (np.abs(found[:, None, :] - centres[None, :, :]) <= 1).all(-1)
    assert near.any(0).all(), "every planted neuron is found within a voxel"
    match = near.argmax(0)                                                        # the detection of every planted neuron
    nf = CWFA.NeuronFootprints(coords, F.SHAPE, "cuda")
    for t in range(0, T, 8):
        nf.update(xd[t:t + 8])
    fp = nf.finish(0.5)
    parts = [CWFA.extract_traces(xd[t:t + 8], fp, nf.geometry, alpha=0.7) for t in range(0, T, 8)]
    Ft, Fnp, Fc = (torch.cat([p[k] for p in parts], dim=1).cpu().numpy() for k in range(3))
    g = nf.geometry
    ref = F.Geometry(found, F.SHAPE)
    assert np.array_equal(g.boxes, ref.boxes) and np.array_equal(g.cores, ref.cores) and np.array_equal(g.occupancy.cpu().numpy(), ref.occ)
    c, u = ops.roi_weighted_sums(xd, g.cores).cpu().numpy(), ops.roi_shell_sums(xd, g)[0].cpu().numpy()
    state = F.accumulate(xh, ref, c, u)
    corr = F.correlate(state[1], state[2], ref, T, True)
    w, wsum, sizes = F.select(corr, ref, 0.5)
    assert same_bits(fp.sizes, sizes) and same_bits(fp.weights, w) and same_bits(fp.wsum, wsum)
    rF, rnp, rFc, bF = F.traces(xh, ref, w, wsum, 0.7)
    ss, smag, counts = F.shell_sums(xh, ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        bnp = (counts[:, None] + 2) * U * smag / counts[:, None]
    bFc = bF + 0.7 * bnp + 2 * U * (np.abs(0.7 * rnp) + np.abs(rFc))
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"seed {seed}: {len(coords)} detections, sizes {sizes.tolist()}; largest error / bound: F {np.nanmax(np.abs(Ft - rF) / bF):.3f}, "
              f"Fnp {np.nanmax(np.abs(Fnp - rnp) / bnp):.3f}, Fc {np.nanmax(np.abs(Fc - rFc) / bFc):.3f}")
    assert within(Ft, rF, bF).all() and within(Fnp, rnp, bnp).all() and within(Fc, rFc, bFc).all()
    r_fc = F.trace_correlations(Fc[match], amp)
    r_box = F.trace_correlations(ops.roi_means(xd, g.boxes).cpu().numpy()[match], amp)
    print(f"seed {seed}: corrected {r_fc.round(3).tolist()}, box mean {r_box.round(3).tolist()}")
    assert (r_fc > r_box).all() and (r_fc > 0.9).all()
