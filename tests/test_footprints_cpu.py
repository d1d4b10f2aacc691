"""CPU: the neuron footprints without a GPU -- the numpy restatement tests/footprints_ref.py against
np.corrcoef and the residual-regression form of the partial correlation, its chunk invariance, geometry, fill and special values; the
purpose of the feature on the scene with a common background; the argument validation of the six entry points through the built
library; and the refusals the Python layer decides before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import footprints_ref as F


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
    return ctypes.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------------------------------------ the restatement
def test_pair_and_partial_correlations():
    """float64 both ways, T = 40: the shifted one-pass sums against numpy's two-pass corrcoef, and the partial correlation against
    the correlation of the residuals of the two regressions on (1, u), to the 1e-12 of section 25."""
    x, geo, c, u = F.small_case()
    T = x.shape[0]
    x0, acc, ref = F.accumulate(x, geo, c, u)
    rie, rig, reg = F.pair_correlations(acc, ref, geo, T)
    r = F.partial_correlations(acc, ref, geo, T)
    X = x.reshape(T, -1).astype(np.float64)
    A = np.stack([np.ones(T), u[0]], axis=1)
    res = lambda y: y - A @ np.linalg.lstsq(A, y, rcond=None)[0]
    worst = [0.0, 0.0, 0.0]
    for i in range(X.shape[1]):
        worst[0] = max(worst[0], abs(rie[i] - np.corrcoef(X[:, i], c[0])[0, 1]))
        worst[1] = max(worst[1], abs(rig[i] - np.corrcoef(X[:, i], u[0])[0, 1]))
        worst[2] = max(worst[2], abs(r[i] - np.corrcoef(res(X[:, i]), res(c[0]))[0, 1]))
    print(f"largest differences: voxel-seed {worst[0]:.2e}, voxel-neuropil {worst[1]:.2e}, partial {worst[2]:.2e}")
    assert abs(reg[0] - np.corrcoef(c[0], u[0])[0, 1]) <= 1e-12
    assert max(worst) <= 1e-12
    assert np.array_equal(F.correlate(acc, ref, geo, T, False), rie.astype(np.float32))


@pytest.mark.parametrize("with_u", [True, False])
def test_the_state_does_not_depend_on_the_chunking(with_u):
    x, geo, c, u = F.small_case(T=9)
    u = u if with_u else None
    whole = F.accumulate(x, geo, c, u)
    for cuts in ((1,) * 9, (4, 5), (1, 2, 6), (8, 1)):
        state, t = None, 0
        for n in cuts:
            state = F.accumulate(x[t:t + n], geo, c[:, t:t + n], None if u is None else u[:, t:t + n], state)
            t += n
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(state, whole)), cuts
    if not with_u:
        assert not whole[1][3].any() and not whole[2][:, [1, 4, 5, 6]].any(), "without neuropil su, u0, g1, g2, eg stay 0.0"


def test_geometry_tables():
    from cwfa_amd import ops
    g = F.Geometry([(0, 0, 0)], (1, 1, 1))
    assert g.boxes.tolist() == [[0, 1, 0, 1, 0, 1]] and g.cores.tolist() == g.boxes.tolist()
    assert g.outer.tolist() == g.inner.tolist() == g.boxes.tolist() and g.offsets.tolist() == [0, 1] and not g.shell(0).any()
    shape = (14, 56, 64)
    centres = [(1, 2, 62), (7, 28, 32), (7, 28, 36), (20, 28, 32)]                  # a corner, two that overlap, one outside in z
    g = F.Geometry(centres, shape)
    assert g.boxes.tolist() == [[0, 4, 0, 7, 57, 64], [4, 10, 23, 33, 27, 37], [4, 10, 23, 33, 31, 41], [0, 0, 23, 33, 27, 37]]
    assert g.cores.tolist() == [[0, 3, 1, 4, 61, 64], [6, 9, 27, 30, 31, 34], [6, 9, 27, 30, 35, 38], [0, 0, 23, 23, 27, 27]]
    assert g.outer.tolist() == [[0, 7, 0, 13, 51, 64], [1, 13, 17, 39, 21, 43], [1, 13, 17, 39, 25, 47], [0] * 6]
    assert g.inner.tolist() == [[0, 5, 0, 9, 55, 64], [3, 11, 21, 35, 25, 39], [3, 11, 21, 35, 29, 43], [0] * 6]
    assert g.offsets.tolist() == [0, 196, 796, 1396, 1396] and g.V == 1396
    assert g.occ.sum() == 196 + 600 + 600 - 6 * 10 * 6, "overlapping boxes are marked once"
    assert g.shell(0).sum() == 7 * 13 * 13 - 5 * 9 * 9 and g.shell(3).sum() == 0
    assert g.shell(1).sum() == 12 * 22 * 22 - 8 * 14 * 14 - 6 * 10 * 2, "the part of the neighbour's box outside the own inner box is taken out"
    mine = ops.footprint_geometry(g.boxes, g.cores, shape, F.GAP, F.ANNULUS, device="cpu")
    assert mine.N == 4 and mine.V == g.V and np.array_equal(mine.offsets, g.offsets) and mine.offsets.dtype == np.int64
    assert np.array_equal(mine.shell_outer, g.outer) and np.array_equal(mine.shell_inner, g.inner) and mine.boxes.dtype == np.int32


@pytest.mark.parametrize("name", ["island", "diagonal", "core_below", "serpentine"])
def test_fill_on_hand_made_maps(name):
    above, core, want = F.fill_case(name)
    geo, corr = F.box_case(above, core)
    w, wsum, sizes = F.select(corr, geo, 0.5)
    got = F.dense(w, geo, 0)
    assert np.array_equal(got != 0, want) and sizes[0] == want.sum()
    assert np.array_equal(got[want], np.full(want.sum(), 0.75, dtype=np.float32)) and wsum[0] == 0.75 * want.sum()
    if name == "serpentine":
        assert want.sum() == 5 * 9 + 4 and want[0, 4, 4]
    if name == "core_below":
        assert sizes[0] == 0 and wsum[0] == 0.0 and not w.any()


def test_special_values():
    x, geo, c, u, planted = F.special_case()
    clean = F.small_case(T=6, seed=4)[0]
    for neuropil in (True, False):
        uu = u if neuropil else None
        ref_corr = F.correlate(*F.accumulate(clean, geo, c, uu)[1:], geo, 6, neuropil)
        corr = F.correlate(*F.accumulate(x, geo, c, uu)[1:], geo, 6, neuropil)
        assert not np.isnan(corr).any() and not corr[planted].any(), "a degenerate voxel has corr 0, never NaN"
        rest = np.setdiff1d(np.arange(geo.V), planted)
        assert np.array_equal(corr[rest].view(np.uint32), ref_corr[rest].view(np.uint32)) and ref_corr[planted].all(), "and only that voxel"
        for bad in (np.nan, np.inf, -np.inf):
            cb = c.copy()
            cb[0, 2] = bad
            assert not F.correlate(*F.accumulate(clean, geo, cb, uu)[1:], geo, 6, neuropil).any(), "a degenerate seed trace: all 0"
        one = F.correlate(*F.accumulate(clean[:1], geo, c[:, :1], None if uu is None else uu[:, :1])[1:], geo, 1, neuropil)
        assert not one.any() and not np.isnan(one).any(), "T = 1"
    ub = u.copy()
    ub[0, 3] = np.nan
    with_bad_u = F.correlate(*F.accumulate(clean, geo, c, ub)[1:], geo, 6, True)
    plain = F.correlate(*F.accumulate(clean, geo, c, None)[1:], geo, 6, False)
    assert np.array_equal(with_bad_u.view(np.uint32), plain.view(np.uint32)), "a degenerate neuropil trace leaves the plain correlation"


# ------------------------------------------------------------------------------------------------ what the feature is for
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_corrected_footprint_trace_follows_the_neuron_where_the_box_mean_does_not(seed):
    x, centres, amp = F.scene(seed, 0.05)
    geo = F.Geometry(centres, F.SHAPE)
    corr, w, wsum, sizes = F.footprints(x, geo, True, 0.5, chunk=8)
    Fc = F.traces(x, geo, w, wsum, 0.7)[2]
    r_fc, r_box = F.trace_correlations(Fc, amp), F.trace_correlations(F.box_means(x, geo.boxes), amp)
    print(f"seed {seed}, bg 0.05: sizes {sizes.tolist()}, corrected {r_fc.round(3).tolist()}, box mean {r_box.round(3).tolist()}")
    assert (r_fc > r_box).all() and (r_fc > 0.9).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_strong_background_swallows_the_box_without_the_neuropil_term(seed):
    x, centres, amp = F.scene(seed, 0.4)
    geo = F.Geometry(centres, F.SHAPE)
    with_np, without = F.footprints(x, geo, True, 0.5)[3], F.footprints(x, geo, False, 0.5)[3]
    print(f"seed {seed}, bg 0.4: sizes with the neuropil term {with_np.tolist()}, without {without.tolist()}")
    assert (with_np < 600).all() and (with_np > 0).all()
    assert (without == 600).any()


# ------------------------------------------------------------------------------------------------ the entry points' arguments
BOX = np.array([[0, 2, 0, 2, 0, 2]], dtype=np.int32)
OFF = np.array([0, 8], dtype=np.int64)
BAD_BOXES = [[0, 3, 0, 2, 0, 2], [-1, 2, 0, 2, 0, 2], [1, 0, 0, 2, 0, 2], [0, 2, 0, 2, 1, 3]]


def test_roi_mark_arguments(built_lib, ptr):
    L = built_lib
    call = lambda boxes=BOX, N=1, occ=ptr, shape=(2, 2, 2): L.cwfa_roi_mark_u8(None if boxes is None else host(boxes), N, occ, *shape, None)
    assert call(occ=None) == -1 and b"cwfa_roi_mark_u8: null" in L.cwfa_last_error()
    assert call(boxes=None) == -1 and call(N=-1) == -2 and call(shape=(2, -2, 2)) == -2
    assert call(shape=((1 << 31) - 1,) * 3, N=0) == -2 and b"2^40" in L.cwfa_last_error()
    for b in BAD_BOXES:
        assert call(np.array([b], dtype=np.int32)) == -1 and b"not inside" in L.cwfa_last_error()
    assert call(np.zeros((1, 6), dtype=np.int32), shape=(0, 2, 2)) == 0 and call(None, 0, None, (2, 0, 2)) == 0, "empty: no device work"


def test_roi_weighted_sums_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(3)]

    def call(x=q[0], boxes=BOX, off=OFF, w=q[1], out=q[2], T=1, shape=(2, 2, 2), N=1, ss=8):
        return L.cwfa_roi_weighted_sums_f32(x, None if boxes is None else host(boxes), None if off is None else host(off), w, out, T, *shape,
                                            N, ss, None)
    assert call(x=None) == -1 and call(out=None) == -1 and call(boxes=None) == -1 and call(off=None) == -1
    assert b"cwfa_roi_weighted_sums_f32: null" in L.cwfa_last_error()
    assert call(T=-1) == -2 and call(N=-1) == -2 and call(shape=(2, 2, -1)) == -2
    assert call(T=2, ss=7) == -1 and b"stride" in L.cwfa_last_error()
    assert call(out=ctypes.c_void_p(q[2].value + 4)) == -3
    for b in BAD_BOXES:
        assert call(boxes=np.array([b], dtype=np.int32)) == -1 and b"not inside" in L.cwfa_last_error()
    assert call(off=np.array([0, 7], dtype=np.int64)) == -1 and b"offsets" in L.cwfa_last_error()
    assert call(off=np.array([1, 9], dtype=np.int64)) == -1 and b"offsets[0]" in L.cwfa_last_error()
    assert call(T=0) == 0 and call(N=0, boxes=None, off=np.zeros(1, dtype=np.int64)) == 0 and call(T=0, w=None, off=None) == 0


def test_roi_shell_sums_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(4)]

    def call(a=q, outer=BOX, inner=BOX, T=1, shape=(2, 2, 2), N=1, ss=8):
        return L.cwfa_roi_shell_sums_f32(a[0], None if outer is None else host(outer), None if inner is None else host(inner), a[1], a[2],
                                         a[3], T, *shape, N, ss, None)
    for k in range(4):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_roi_shell_sums_f32: null" in L.cwfa_last_error()
    assert call(outer=None) == -1 and call(inner=None) == -1
    assert call(T=-1) == -2 and call(N=-1) == -2 and call(shape=(-2, 2, 2)) == -2
    assert call(T=3, ss=7) == -1 and b"stride" in L.cwfa_last_error()
    odd = list(q)
    odd[2] = ctypes.c_void_p(q[2].value + 4)
    assert call(odd) == -3
    for b in BAD_BOXES:
        bad = np.array([b], dtype=np.int32)
        assert call(outer=bad) == -1 and b"outer box" in L.cwfa_last_error()
        assert call(inner=bad) == -1 and b"inner box" in L.cwfa_last_error()
    assert call(T=0) == 0 and call(N=0, outer=None, inner=None) == 0


def test_footprint_update_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(6)]                 # x, c, u, x0, acc, ref

    def call(a=q, boxes=BOX, off=OFF, T=1, shape=(2, 2, 2), N=1, ss=8, first=1):
        return L.cwfa_footprint_update_f32(a[0], None if boxes is None else host(boxes), None if off is None else host(off), a[1], a[2],
                                           a[3], a[4], a[5], T, *shape, N, ss, first, None)
    for k in (0, 1, 3, 4, 5):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_footprint_update_f32: null" in L.cwfa_last_error()
    assert call(boxes=None) == -1 and call(off=None) == -1
    assert call(T=-1, first=0) == -2 and call(N=-1) == -2 and call(shape=(2, -2, 2)) == -2
    assert call(T=0) == -2 and b"first chunk" in L.cwfa_last_error()
    assert call(first=2) == -1
    assert call(T=2, ss=7) == -1 and b"stride" in L.cwfa_last_error()
    for b in BAD_BOXES:
        assert call(boxes=np.array([b], dtype=np.int32)) == -1 and b"not inside" in L.cwfa_last_error()
    assert call(off=np.array([0, 9], dtype=np.int64)) == -1 and b"offsets" in L.cwfa_last_error()
    for k in (1, 2, 4, 5):
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert call(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    assert call(T=0, first=0) == 0 and call(boxes=None, off=np.zeros(1, dtype=np.int64), N=0) == 0, "empty: no launch"


def test_footprint_corr_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(3)]                 # acc, ref, corr
    call = lambda a=q, off=OFF, N=1, T=3, np_=1: L.cwfa_footprint_corr_f32(a[0], a[1], None if off is None else host(off), N, T, np_, a[2], None)
    for k in range(3):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_footprint_corr_f32: null" in L.cwfa_last_error()
    assert call(off=None) == -1 and call(N=-1) == -2 and call(T=0) == -2 and call(T=1 << 31) == -2 and call(np_=2) == -1
    assert call(off=np.array([0, -1], dtype=np.int64)) == -1 and call(off=np.array([2, 8], dtype=np.int64)) == -1
    for k in range(2):
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert call(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    assert call(off=np.zeros(1, dtype=np.int64), N=0) == 0 and call(off=np.zeros(2, dtype=np.int64)) == 0, "no state voxel: no launch"


def test_footprint_select_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(4)]                 # corr, w, wsum, size
    core = np.array([[0, 1, 0, 1, 0, 1]], dtype=np.int32)

    def call(a=q, boxes=BOX, cores=core, off=OFF, N=1, thr=0.5):
        h = lambda t: None if t is None else host(t)
        return L.cwfa_footprint_select_f32(a[0], h(boxes), h(cores), h(off), N, thr, a[1], a[2], a[3], None)
    for k in range(4):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_footprint_select_f32: null" in L.cwfa_last_error()
    assert call(boxes=None) == -1 and call(cores=None) == -1 and call(off=None) == -1 and call(N=-1) == -2
    for thr in (0.0, -0.5, 1.5, float("nan")):
        assert call(thr=thr) == -1 and b"thr" in L.cwfa_last_error()
    for c in ([0, 3, 0, 1, 0, 1], [1, 0, 0, 1, 0, 1], [0, 1, -1, 1, 0, 1]):
        assert call(cores=np.array([c], dtype=np.int32)) == -1 and b"core" in L.cwfa_last_error()
    assert call(boxes=np.array([[2, 0, 0, 2, 0, 2]], dtype=np.int32)) == -1
    assert call(off=np.array([0, 7], dtype=np.int64)) == -1 and b"offsets" in L.cwfa_last_error()
    big = np.array([[0, 32, 0, 32, 0, 33]], dtype=np.int32)
    assert call(boxes=big, off=np.array([0, 32 * 32 * 33], dtype=np.int64)) == -2 and b"2^15" in L.cwfa_last_error()
    odd = list(q)
    odd[2] = ctypes.c_void_p(q[2].value + 4)
    assert call(odd) == -3
    assert call(boxes=None, cores=None, off=np.zeros(1, dtype=np.int64), N=0) == 0


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_the_python_layer_refuses_before_any_device_work(built_lib):
    from cwfa_amd import CWFA, _lib, ops
    assert _lib.FOOTPRINT_SELECT_MAX == 1 << 15
    assert {"NeuronFootprints", "Footprints", "extract_traces"} <= set(CWFA.__all__)
    shape = (14, 56, 64)
    shift = shape[0] // 2 + (-25 // 2)
    coords = [[32, 28, 7 - shift], [62, 2, 1 - shift]]
    nf = CWFA.NeuronFootprints(coords, shape, "cpu")
    want = F.Geometry([(7, 28, 32), (1, 2, 62)], shape)
    g = nf.geometry
    assert np.array_equal(g.boxes, want.boxes) and np.array_equal(g.cores, want.cores) and np.array_equal(g.offsets, want.offsets)
    assert np.array_equal(g.shell_outer, want.outer) and np.array_equal(g.shell_inner, want.inner)
    assert nf.count == 0 and nf.neuropil and nf.state[0].shape == (want.V,) and nf.state[1].shape == (4, want.V) and nf.state[2].shape == (2, 7)
    assert nf.state[1].dtype == torch.float64 and nf.state[0].dtype == torch.float32
    for bad in ({"gap": (1, -2, 2)}, {"annulus": (2, 4, -4)}, {"core": (-1, 1, 1)}, {"gap": (1, 2)}, {"r12": 0}):
        with pytest.raises(ValueError):
            CWFA.NeuronFootprints(coords, shape, "cpu", **bad)
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        CWFA.NeuronFootprints(coords, (56, 64), "cpu")
    with pytest.raises(ValueError, match="no volume"):
        nf.finish()
    for thr in (0.0, 1.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match="thr"):
            nf.finish(thr)
        with pytest.raises(ValueError, match="thr"):
            ops.footprint_select(torch.zeros(g.V), g, thr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nf.update(torch.zeros(2, *shape))
    with pytest.raises(ValueError, match="inside the volume"):
        ops.footprint_geometry([[0, 15, 0, 2, 0, 2]], [[0, 1, 0, 1, 0, 1]], shape)
    with pytest.raises(ValueError, match="inside its box"):
        ops.footprint_geometry([[0, 2, 0, 2, 0, 2]], [[0, 3, 0, 1, 0, 1]], shape)
    with pytest.raises(ValueError, match="one core per box"):
        ops.footprint_geometry([[0, 2, 0, 2, 0, 2]], np.zeros((0, 6), dtype=np.int32), shape)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.roi_mark(g.boxes, shape, "cpu")
    with pytest.raises(ValueError, match="inside the volume"):
        ops.roi_mark([[0, 2, 0, 2, 0, 65]], shape, "cpu")
    x = torch.zeros(2, *shape)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.roi_weighted_sums(x, g.boxes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.roi_shell_sums(x, g)
    with pytest.raises(ValueError, match="FootprintGeometry"):
        ops.roi_shell_sums(x, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.footprint_update(x, g, torch.zeros(2, 2, dtype=torch.float64), None, nf.state, True)
    with pytest.raises(ValueError, match="HIP device"):
        ops.footprint_corr(nf.state, g, 2)
    with pytest.raises(ValueError, match="what NeuronFootprints.finish returns"):
        CWFA.extract_traces(x, None)
    fp = CWFA.Footprints(g.boxes, g.offsets, torch.zeros(g.V), torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), torch.zeros(g.V))
    assert fp.dense(0).shape == (6, 10, 10) and fp.dense(1).shape == (4, 7, 7)
    with pytest.raises(ValueError, match="FootprintGeometry or None"):
        CWFA.extract_traces(x, fp, geometry=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CWFA.extract_traces(x, fp, g)
