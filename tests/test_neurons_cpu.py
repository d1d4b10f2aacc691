"""CPU: neuron detection without a GPU -- the numpy restatement tests/neurons_ref.py on hand-made maps and on the
planted scene, the argument validation of the three new entry points through the built library, the coordinates file against the
fixture the reference's reader produced, and the refusals ``find_neurons`` decides before any device work."""
import ctypes
import os

import numpy as np
import pytest
import torch

import neurons_ref as R
from conftest import load_golden


@pytest.fixture(scope="module")
def L():
    from cwfa_amd import _lib, build
    build.build_all()
    return _lib.lib()


@pytest.fixture(scope="module")
def ptr():
    buf = ctypes.create_string_buffer(16384)
    base = ctypes.addressof(buf)
    return ctypes.c_void_p((base + 15) & ~15)


# ------------------------------------------------------------------------------------------------ the restatement
def test_keys_order_like_the_values_with_ties_to_the_lower_index():
    v = np.array([np.nan, -np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], dtype=np.float32)
    o = R.ord32(v).astype(np.int64)
    assert o[0] == 0 and o[4] == o[5], "NaN is below everything; -0 and +0 are one value"
    assert np.all(np.diff(np.delete(o, 4)) > 0)
    k = R.keys(np.zeros((1, 2, 3), dtype=np.float32)).reshape(-1)
    assert np.all(k[:-1] > k[1:]), "equal values: the lower index has the higher key"


def test_a_plateau_yields_its_first_voxel_and_a_margin_removes_it():
    s = np.zeros((4, 8, 8), dtype=np.float32)
    s[1:3, 2:6, 2:6] = 1.0                                                   # a 2 x 4 x 4 plateau
    zyx, sc, total = R.local_maxima(s, 0.5, (1, 1, 1))
    assert total == 1 and zyx.tolist() == [[1, 2, 2]] and sc.tolist() == [1.0]
    assert R.local_maxima(s, 0.5, (1, 1, 1), margin=(0, 3, 0))[2] == 0, "(1,2,2) lies 2 from the y face"
    assert R.local_maxima(s, 0.5, (1, 1, 1), margin=(1, 2, 2))[0].tolist() == [[1, 2, 2]]
    # inside the margin a voxel still suppresses: the plateau's other voxels do not take over
    assert R.local_maxima(s, 0.5, (1, 1, 1), margin=(0, 3, 3))[2] == 0
    # dist 0: every voxel at or above the threshold, by index
    zyx, _, total = R.local_maxima(s, 0.5, (0, 0, 0))
    assert total == 32 and zyx[0].tolist() == [1, 2, 2] and zyx[-1].tolist() == [2, 5, 5]
    assert R.local_maxima(s, 0.5, (0, 0, 0), n_max=5)[0].shape == (5, 3) and R.local_maxima(s, 0.5, (0, 0, 0), n_max=5)[2] == 32
    assert R.local_maxima(s, 2.0, (1, 1, 1))[2] == 0 and R.local_maxima(s, 2.0, (1, 1, 1))[0].shape == (0, 3)


def test_special_values():
    s = np.full((1, 1, 9), -1.0, dtype=np.float32)
    s[0, 0, 1], s[0, 0, 4], s[0, 0, 7] = np.nan, np.inf, -np.inf
    zyx, sc, total = R.local_maxima(s, -np.inf, (0, 0, 1))
    assert zyx[:, 2].tolist() == [4, 0, 2, 8] and total == 4, "inf, then the -1 that lead their windows: beside NaN (twice) and beside -inf"
    assert sc[0] == np.inf and sc[1:].tolist() == [-1.0] * 3
    z = np.array([[[-0.0, 0.0, 0.0]]], dtype=np.float32)
    assert R.local_maxima(z, 0.0, (0, 0, 2))[0].tolist() == [[0, 0, 0]], "-0.0 ties with +0.0 and wins by index"


@pytest.mark.parametrize("seed", range(5))
def test_the_scene_is_recovered_exactly(seed):
    """The condition the GPU end-to-end test is held to, on the CPU: the unbiased temporal std of the scene has exactly the planted
    centres as peaks."""
    stack, centres = R.scene(seed)
    score = stack.astype(np.float64).std(0, ddof=1).astype(np.float32)
    zyx, sc, total = R.local_maxima(score, 0.1, (5, 9, 9))
    assert total == 24 and sorted(map(tuple, zyx.tolist())) == sorted(map(tuple, centres.tolist()))
    print(f"seed {seed}: lowest peak score {sc.min():.3f}, median of the map {np.median(score):.4f}")
    assert sc.min() >= 0.3 and np.median(score) <= 0.005
    assert R.far_apart(zyx, (5, 9, 9))
    from cwfa_amd.CWFA import roi_boxes
    shift = score.shape[0] // 2 - 13
    coords = [[int(x), int(y), int(z) - shift] for z, y, x in zyx]
    boxes = roi_boxes(coords, (1,) + score.shape, 5, 3)
    assert R.boxes_disjoint(boxes), "dist = (2 r3 - 1, 2 r12 - 1, 2 r12 - 1): the ROIs [c - r, c + r) cannot overlap"
    for (z, y, x), b in zip(zyx, boxes):
        assert b[0] <= z < b[1] and b[2] <= y < b[3] and b[4] <= x < b[5]


def test_separation_on_a_random_map():
    rng = np.random.default_rng(1)
    s = rng.random((9, 40, 33)).astype(np.float32)
    for dist in ((1, 2, 3), (0, 9, 1), (16, 16, 16)):
        zyx, sc, total = R.local_maxima(s, 0.0, dist)
        assert total >= 1 and R.far_apart(zyx, dist) and np.all(np.diff(sc) <= 0)
    assert not R.far_apart([[0, 0, 0], [1, 2, 3]], (1, 2, 3)) and R.far_apart([[0, 0, 0], [1, 2, 4]], (1, 2, 3))
    assert R.boxes_disjoint([[0, 2, 0, 2, 0, 2], [0, 2, 0, 2, 2, 4]]) and not R.boxes_disjoint([[0, 2, 0, 2, 0, 2], [1, 3, 1, 3, 1, 3]])


# ------------------------------------------------------------------------------------------------ the entry points' arguments
def test_activity_update_arguments(L, ptr):
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(6)]
    for k in range(6):
        args = list(q)
        args[k] = None
        assert L.cwfa_activity_update_f32(*args, 1, 8, 8, 1, None) == -1 and b"cwfa_activity_update_f32: null" in L.cwfa_last_error()
    assert L.cwfa_activity_update_f32(*q, -1, 8, 8, 0, None) == -2 and L.cwfa_activity_update_f32(*q, 1, -8, 8, 0, None) == -2
    assert L.cwfa_activity_update_f32(*q, 2, 8, 7, 0, None) == -1 and b"stride" in L.cwfa_last_error()
    assert L.cwfa_activity_update_f32(*q, 0, 8, 8, 1, None) == -2 and b"first chunk" in L.cwfa_last_error()
    assert L.cwfa_activity_update_f32(*q, 1, 8, 8, 2, None) == -1
    odd = list(q)
    odd[2] = ctypes.c_void_p(q[2].value + 4)
    assert L.cwfa_activity_update_f32(*odd, 1, 8, 8, 1, None) == -3 and b"8-byte" in L.cwfa_last_error()
    assert L.cwfa_activity_update_f32(*q, 0, 8, 8, 0, None) == 0 and L.cwfa_activity_update_f32(*q, 3, 0, 0, 1, None) == 0, "empty: no launch"


def test_activity_finish_arguments(L, ptr):
    q = [ctypes.c_void_p(ptr.value + 1024 * k) for k in range(8)]
    call = lambda a, N=3, kind=0, m=8: L.cwfa_activity_finish_f32(*a[:5], N, kind, *a[5:], m, None)
    for k in range(8):
        args = list(q)
        args[k] = None
        assert call(args) == -1 and b"cwfa_activity_finish_f32: null" in L.cwfa_last_error()
    assert call(q, kind=4) == -1 and call(q, kind=-1) == -1 and b"unknown kind" in L.cwfa_last_error()
    assert call(q, N=0) == -2 and call(q, N=1 << 31) == -2 and call(q, m=-1) == -2
    odd = list(q)
    odd[1] = ctypes.c_void_p(q[1].value + 4)
    assert call(odd) == -3
    assert call(q, m=0) == 0


def test_local_maxima_arguments(L, ptr):
    s, ws, out, cnt = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(4))
    call = lambda score=s, shape=(2, 4, 4), dist=(1, 1, 1), margin=(0, 0, 0), w=ws, o=out, cap=4, c=cnt: \
        L.cwfa_local_maxima_f32(score, *shape, 0.5, *dist, *margin, w, o, cap, c, None)
    assert call(score=None) == -1 and call(w=None) == -1 and call(o=None) == -1 and call(c=None) == -1
    assert b"cwfa_local_maxima_f32: null" in L.cwfa_last_error()
    for shape in ((-1, 4, 4), (2, -4, 4), (2, 4, -4)):
        assert call(shape=shape) == -2
    assert call(cap=-1) == -1 and call(margin=(0, -1, 0)) == -1
    for dist in ((17, 1, 1), (1, 17, 1), (1, 1, 17), (-1, 1, 1), (1, 1, -1)):
        assert call(dist=dist) == -2 and b"half-widths" in L.cwfa_last_error(), dist
    for shape in ((65536, 65536, 2), (3, 1 << 30, 2), (1, 1 << 30, 1 << 30), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)):
        assert call(shape=shape) == -2 and b"32-bit linear index" in L.cwfa_last_error(), shape
    assert call(w=ctypes.c_void_p(ws.value + 4)) == -3 and call(c=ctypes.c_void_p(cnt.value + 4)) == -3


# ------------------------------------------------------------------------------------------------ the coordinates file
def test_csv_round_trip_against_the_reference_readers_result(tmp_path):
    from cwfa_amd import CWFA
    fx = load_golden("g27_neuron_coords")
    paths = []
    for name in fx["sets"]:
        coords = fx[f"{name}/coords"].tolist()
        scores = fx[f"{name}/scores"].tolist() if f"{name}/scores" in fx else None
        path = str(tmp_path / f"{name}.csv")
        assert CWFA.write_neural_coordinates_to_file(coords, path, scores) == path
        text = open(path).read()
        assert text == str(fx[f"{name}/csv"]), "the writer's text is the one the reference's reader was given"
        header = text.splitlines()[0].split(",")
        assert header == ["patch_n", "coord_x", "coord_y", "coord_z", "corr_coeff", "is_gt"] + (["score"] if scores else [])
        got = CWFA.read_neural_coordinates_from_file(path)
        assert got == coords and all(type(v) is int for row in got for v in row)
        paths.append(path)
    assert min(c[2] for c in fx["plain/coords"].tolist()) < 0, "a negative relative z is in the fixture"
    # the documented departure: a list of files gives the rows of all of them (the reference: the first file's, or no result at all)
    both = CWFA.read_neural_coordinates_from_file(paths)
    assert both == fx["plain/coords"].tolist() + fx["scored/coords"].tolist()
    if int(fx["list/raised"]) == 0:
        assert fx["list/coords"].tolist() == fx["plain/coords"].tolist()
    # rows with is_gt != 1 are not coordinates
    mixed = str(tmp_path / "mixed.csv")
    open(mixed, "w").write("patch_n,coord_x,coord_y,coord_z,corr_coeff,is_gt\n0,1,2,3,0.5,1\n0,1,2,3,0.5,0\n1,4,5,-6,0.1,1\n")
    assert CWFA.read_neural_coordinates_from_file(mixed) == [[1, 2, 3], [4, 5, -6]]
    with pytest.raises(ValueError, match="integer rows"):
        CWFA.write_neural_coordinates_to_file([[1.5, 2, 3]], mixed)
    with pytest.raises(ValueError, match="one score per coordinate"):
        CWFA.write_neural_coordinates_to_file([[1, 2, 3]], mixed, [1.0, 2.0])
    assert not os.path.exists(str(tmp_path / "never.csv"))


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_find_neurons_refuses_bad_arguments_before_any_device_work():
    from cwfa_amd import CWFA, ops
    s = torch.zeros(4, 8, 8)
    for kw, msg in ((dict(r12=0), "positive"), (dict(r3=0), "positive"), (dict(dist=(17, 1, 1)), "half-widths"),
                    (dict(dist=(1, 1)), "three integers"), (dict(dist=(1, 1.5, 1)), "three integers"), (dict(margin=(0, -1, 0)), "not negative"),
                    (dict(n_max=-1), "not negative"), (dict(rel_thr=1.5), "rel_thr"), (dict(rel_thr=-0.1), "rel_thr"),
                    (dict(r12=9), "half-widths")):
        with pytest.raises(ValueError, match=msg):
            CWFA.find_neurons(s, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CWFA.find_neurons(s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.local_maxima(s, 0.5, (1, 1, 1))
    with pytest.raises(ValueError, match="half-widths"):
        ops.local_maxima(s, 0.5, (1, 1, 17))
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        CWFA.ActivityMap((4, 8), "cpu")
    with pytest.raises(ValueError, match="kind"):
        ops.activity_finish((s,) * 5, 3, kind="variance")
    assert CWFA.find_neurons.__defaults__[5] == -13 and {"ActivityMap", "find_neurons", "read_neural_coordinates_from_file",
                                                          "write_neural_coordinates_to_file"} <= set(CWFA.__all__)
