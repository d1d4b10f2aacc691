"""CPU: the streaming local-correlation map without a GPU -- the numpy restatement tests/corrmap_ref.py against
np.corrcoef, its neighbourhoods and special values, the purpose of the feature on the scene with hot voxels, the argument validation
of the two new entry points through the built library, and the refusals the Python layer decides before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import corrmap_ref as C
import neurons_ref as R


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


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("neighbours", [6, 8, 26])
def test_pair_correlations_are_corrcoef(neighbours):
    """float64 both ways, T = 40: the shifted one-pass form against numpy's two-pass one to 1e-12 (the series are O(1) with a mean of
    3: the shift by x(0) keeps the cancellation in s2 - s1^2 / N at a few hundred ulp at most)."""
    rng = np.random.default_rng(3)
    x = (3.0 + rng.standard_normal((40, 3, 4, 5))).astype(np.float32)
    x0, s1, s2, cc = C.accumulate(x, neighbours)
    rs, inside = C.pair_correlations(s1, s2, cc, 40, neighbours)
    worst = 0.0
    for o in C.offsets(neighbours):
        for z, y, xx in zip(*np.nonzero(inside[o])):
            j = (z + o[0], y + o[1], xx + o[2])
            want = np.corrcoef(x[:, z, y, xx].astype(np.float64), x[(slice(None), *j)].astype(np.float64))[0, 1]
            worst = max(worst, abs(rs[o][z, y, xx] - want))
    print(f"{neighbours} neighbours: largest difference from np.corrcoef {worst:.2e}")
    assert worst <= 1e-12
    sc, n = C.finish(s1, s2, cc, 40, neighbours)
    mean = sum(rs[o] for o in C.offsets(neighbours)) / n
    assert sc.dtype == np.float32 and np.abs(sc - mean).max() <= 1e-6 and np.abs(sc).max() <= 1.0


def test_offsets_and_neighbour_counts():
    assert C.forward(6) == [(0, 0, 1), (0, 1, 0), (1, 0, 0)]
    assert C.forward(8) == [(0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1)]
    assert C.forward(26) == [(0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1), (1, -1, -1), (1, -1, 0), (1, -1, 1), (1, 0, -1), (1, 0, 0), (1, 0, 1),
                             (1, 1, -1), (1, 1, 0), (1, 1, 1)]
    for nb, K in ((6, 3), (8, 4), (26, 13)):
        all_ = C.offsets(nb)
        assert len(all_) == nb and all_ == sorted(all_) and len(C.forward(nb)) == K
        assert all_ == [tuple(-a for a in o) for o in reversed(C.forward(nb))] + C.forward(nb), "backward half, then forward half"
    rng = np.random.default_rng(0)

    def counts(shape, nb):
        x = rng.standard_normal((5, *shape)).astype(np.float32)
        x0, s1, s2, cc = C.accumulate(x, nb)
        sc, n = C.finish(s1, s2, cc, 5, nb)
        return sc, n, cc

    for nb in (6, 8, 26):
        sc, n, cc = counts((1, 1, 1), nb)
        assert n.tolist() == [[[0]]] and sc.tolist() == [[[0.0]]] and not cc.any(), "no neighbour at all: the score is 0"
    sc, n, cc = counts((3, 4, 1), 26)                                          # W = 1: nothing along x
    assert n[1, 1, 0] == 8 and n[0, 0, 0] == 3 and n.max() == 8
    assert all(not cc[k].any() for k, o in enumerate(C.forward(26)) if o[2] != 0), "a row's last voxel has no +x neighbour"
    assert counts((3, 4, 1), 6)[1][1, 1, 0] == 4 and counts((3, 4, 1), 8)[1][1, 1, 0] == 2
    sc, n, cc = counts((3, 4, 5), 26)
    assert n[1, 1, 1] == 26 and n[0, 0, 0] == 7 and n[0, 1, 1] == 17 and n[0, 0, 1] == 11
    assert counts((3, 4, 5), 6)[1][0, 0, 0] == 3 and counts((3, 4, 5), 8)[1][0, 0, 0] == 3 and counts((1, 4, 5), 8)[1][0, 1, 1] == 8
    k = C.forward(26).index((0, 0, 1))
    assert not cc[k][:, :, -1].any() and cc[k][:, :, :-1].all(), "the pair sum is 0.0 exactly where the neighbour is outside"
    k = C.forward(26).index((1, -1, 1))
    assert not cc[k][-1].any() and not cc[k][:, 0].any() and not cc[k][:, :, -1].any() and cc[k][:-1, 1:, :-1].all()


@pytest.mark.parametrize("neighbours", [6, 8, 26])
def test_special_values(neighbours):
    """A constant voxel, NaN, +inf, -inf (also as the first sample) and N = 1: r = 0 for every pair they are in, never NaN."""
    x, y, planted = C.special_stack()
    clean = C.score(x, neighbours)
    sc = C.score(y, neighbours)
    assert not np.isnan(sc).any() and np.abs(sc).max() <= 1.0
    touched = C.touched(planted, sc.shape, neighbours)
    assert np.array_equal(sc[~touched].view(np.uint32), clean[~touched].view(np.uint32)), "only the voxel and its neighbours change"
    assert (sc[touched] != clean[touched]).sum() > len(planted)
    x0, s1, s2, cc = C.accumulate(y, neighbours)
    rs, inside = C.pair_correlations(s1, s2, cc, 6, neighbours)
    for c in planted:
        assert all(rs[o][c] == 0.0 for o in C.offsets(neighbours)), "a degenerate voxel's pairs count with r = 0"
    assert sc[1, 1, 1] == 0.0
    one = C.score(x[:1], neighbours)
    assert not one.any() and not np.isnan(one).any(), "N = 1"


# ------------------------------------------------------------------------------------------------ what the feature is for
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_correlation_map_finds_the_neurons_where_the_std_map_finds_hot_voxels(seed):
    stack, centres = C.scene_hot(seed)
    zyx, sc, total = C.scene_peaks(seed)
    print(f"seed {seed}: {total} peaks on the 26-neighbour map, lowest score {sc.min() if total else float('nan'):.3f}")
    assert total == len(centres) == 24
    gap = np.abs(zyx[:, None, :].astype(np.int64) - centres[None, :, :])
    near = (gap <= 1).all(-1)
    assert near.any(1).all() and near.any(0).all(), "every peak within one voxel per axis of a planted centre, and every centre found"
    std = stack.astype(np.float64).std(0, ddof=1).astype(np.float32)
    n_std = R.local_maxima(std, 0.1 * float(std.max()), C.DIST, C.MARGIN)[2]
    print(f"seed {seed}: {n_std} peaks on the std map at rel_thr 0.1")
    assert n_std > 24


# ------------------------------------------------------------------------------------------------ the entry points' arguments
def test_activity_update_corr_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(7)]
    call = lambda a=q, T=1, shape=(2, 2, 2), ss=8, nb=6, first=1: L.cwfa_activity_update_corr_f32(*a, T, *shape, ss, nb, first, None)
    for k in range(7):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_activity_update_corr_f32: null" in L.cwfa_last_error()
    assert call(T=-1, first=0) == -2
    for shape in ((-2, 2, 2), (2, -2, 2), (2, 2, -2)):
        assert call(shape=shape) == -2 and b"negative" in L.cwfa_last_error()
    assert call(shape=((1 << 31) - 1,) * 3) == -2 and b"2^40" in L.cwfa_last_error()
    assert call(T=2, ss=7, first=0) == -1 and b"stride" in L.cwfa_last_error()
    assert call(T=0) == -2 and b"first chunk" in L.cwfa_last_error()
    assert call(first=2) == -1
    for nb in (0, 7, 18, 27, -6):
        assert call(nb=nb) == -1 and b"neighbours" in L.cwfa_last_error()
    for k in (2, 3, 6):
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert call(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    for nb in (6, 8, 26):
        assert call(T=0, first=0, nb=nb) == 0 and call(T=3, shape=(0, 2, 2), nb=nb) == 0 and call(shape=(2, 2, 0), nb=nb) == 0, "empty: no launch"


def test_activity_corr_finish_arguments(built_lib, ptr):
    L = built_lib
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(4)]
    call = lambda a=q, N=3, shape=(2, 2, 2), nb=26: L.cwfa_activity_corr_finish_f32(*a[:3], N, *shape, nb, a[3], None)
    for k in range(4):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_activity_corr_finish_f32: null" in L.cwfa_last_error()
    for nb in (0, 4, 9, 27):
        assert call(nb=nb) == -1 and b"neighbours" in L.cwfa_last_error()
    assert call(N=0) == -2 and call(N=1 << 31) == -2 and call(shape=(2, -1, 2)) == -2
    assert call(shape=((1 << 31) - 1,) * 3) == -2 and b"2^40" in L.cwfa_last_error()
    for k in range(3):
        odd = list(q)
        odd[k] = ctypes.c_void_p(q[k].value + 4)
        assert call(odd) == -3 and b"8-byte" in L.cwfa_last_error()
    assert call(shape=(0, 2, 2)) == 0 and call(shape=(2, 2, 0), nb=6) == 0


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_the_python_layer_refuses_before_any_device_work(built_lib):
    from cwfa_amd import CWFA, _lib, ops
    assert _lib.CORR_FORWARD == {nb: len(C.forward(nb)) for nb in (6, 8, 26)}
    shape = (2, 3, 4)
    state = ops.activity_state(shape, "cpu")
    cc = ops.correlation_state(shape, "cpu", 26)
    assert cc.shape == (13, *shape) and cc.dtype == torch.float64
    assert ops.correlation_state(shape, "cpu", 6).shape[0] == 3 and ops.correlation_state(shape, "cpu", 8).shape[0] == 4
    with pytest.raises(ValueError, match="neighbours"):
        ops.correlation_state(shape, "cpu", 18)
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        ops.correlation_state((3, 4), "cpu", 6)
    x = torch.zeros(2, *shape)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.activity_update_corr(x, state, cc, 26, True)
    with pytest.raises(ValueError, match="HIP device"):
        ops.correlation_finish(state, cc, 2, 26)
    with pytest.raises(ValueError, match="neighbours"):
        ops.correlation_finish(state, cc, 2, 7)
    with pytest.raises(ValueError, match="neighbours is 0, 6, 8 or 26"):
        CWFA.ActivityMap(shape, "cpu", neighbours=18)
    with pytest.raises(ValueError, match="needs an ActivityMap"):
        CWFA.ActivityMap(shape, "cpu").finish("corr")
    with pytest.raises(ValueError, match="needs an ActivityMap"):
        CWFA.find_neurons(CWFA.ActivityMap(shape, "cpu", neighbours=0), kind="corr")
    am = CWFA.ActivityMap(shape, "cpu", neighbours=8)
    assert am.neighbours == 8 and am.cc.shape == (4, *shape) and CWFA.ActivityMap(shape, "cpu").cc is None
    with pytest.raises(ValueError, match="no volume"):
        am.finish("corr")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        am.update(x)
    assert CWFA.find_neurons.__defaults__[-1] == "std", "the new keyword is the last one and keeps today's score"
