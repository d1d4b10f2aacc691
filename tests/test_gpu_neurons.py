"""GPU: neuron detection.  The streaming activity map against ops.stack_mean_std and torch.amax / amin of the whole
stack, bit for bit, for every chunking; the four score kinds against the fp32 torch expression, exactly; the detector against the
numpy restatement tests/neurons_ref.py, exactly, on the smallest shapes at which it can go wrong; and frames -> activity map ->
find_neurons -> ROIs -> coordinates file on the planted scene."""
import functools

import numpy as np
import pytest
import torch

import neurons_ref as R

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def stack(shape, T=7, seed=0):
    """A [T, *shape] device stack with a large mean and a small spread, and one constant voxel."""
    g = torch.Generator().manual_seed(seed)
    x = 100.0 + torch.randn(T, *shape, generator=g)
    x[:, 0, 0, 0] = 3.25
    return x.cuda()


def run_map(x, chunks, kind="std"):
    from cwfa_amd.CWFA import ActivityMap
    am = ActivityMap(x.shape[1:], x.device)
    t = 0
    for c in chunks:
        am.update(x[t] if c == 0 else x[t:t + c])               # 0: one volume as [D,H,W]
        t += max(c, 1)
    assert t == x.shape[0] and am.count == t
    return am.finish(kind)


# ------------------------------------------------------------------------------------------------ the accumulator
@pytest.mark.parametrize("shape", [(5, 6, 10), (3, 5, 7)], ids=["m300_vector", "m105_element"])
@pytest.mark.parametrize("chunks", [(1,) * 7, (0,) * 7, (3, 4), (7,), (1, 2, 4), "strided"], ids=str)
def test_activity_map_is_stack_mean_std_bit_for_bit(shape, chunks):
    from cwfa_amd import ops
    x = stack(shape)
    mean, std = ops.stack_mean_std(x)
    if chunks == "strided":                                           # a view with a time stride above a volume: no copy is made
        m = x[0].numel()
        wide = torch.zeros(7, m + 8, device="cuda")
        wide[:, :m] = x.reshape(7, m)
        view = wide.as_strided((7, *shape), (m + 8, shape[1] * shape[2], shape[2], 1))
        assert view.stride(0) == m + 8 and not view.is_contiguous() and torch.equal(view, x)
        score, mo, so, vmax, vmin = run_map(view, (3, 4))
    else:
        score, mo, so, vmax, vmin = run_map(x, chunks)
    assert same_bits(mo, mean) and same_bits(so, std), "mean / std differ from stack_mean_std of the whole stack"
    assert same_bits(vmax, torch.amax(x, 0)) and same_bits(vmin, torch.amin(x, 0))
    assert same_bits(score, so)
    assert float(so[0, 0, 0]) == 0.0 and float(mo[0, 0, 0]) == 3.25, "the constant voxel"
    ref = x.double().std(0)
    assert float(((so.double() - ref).abs() / ref.clamp(min=1e-30))[ref > 0].max()) < 1e-6, "and it is the std"


def test_one_sample_gives_nan_std_and_more_volumes_may_follow():
    from cwfa_amd import ops
    from cwfa_amd.CWFA import ActivityMap
    x = stack((5, 6, 10))
    am = ActivityMap(x.shape[1:], x.device).update(x[:1])
    score, mo, so, vmax, vmin = am.finish()
    assert bool(torch.isnan(so).all()) and bool(torch.isnan(score).all()) and same_bits(mo, x[0]) and same_bits(vmax, x[0]) and same_bits(vmin, x[0])
    m1, s1 = ops.stack_mean_std(x[:1])
    assert same_bits(mo, m1) and same_bits(so, s1)
    am.update(x[1:4])
    am.finish("snr")
    am.update(x[4:])                                                # finish keeps the state
    mean, std = ops.stack_mean_std(x)
    _, mo, so, _, _ = am.finish()
    assert am.count == 7 and same_bits(mo, mean) and same_bits(so, std)
    with pytest.raises(ValueError, match="no volume"):
        ActivityMap((2, 2, 2), "cuda").finish()
    with pytest.raises(ValueError, match="expected"):
        am.update(x[:, :4])


@pytest.mark.parametrize("shape", [(5, 6, 10), (3, 5, 7)], ids=["vector", "element"])
def test_score_kinds_are_the_fp32_expressions(shape):
    x = stack(shape)
    maps = {k: run_map(x, (3, 4), k) for k in ("std", "range", "peak", "snr")}
    _, mean, std, vmax, vmin = maps["std"]
    for k in maps:
        assert all(same_bits(a, b) for a, b in zip(maps[k][1:], maps["std"][1:])), "the maps do not depend on the kind"
    assert same_bits(maps["std"][0], std)
    assert same_bits(maps["range"][0], vmax - vmin)
    assert same_bits(maps["peak"][0], vmax - mean)
    snr = torch.where(std == 0, torch.zeros_like(std), (vmax - mean) / std)
    assert same_bits(maps["snr"][0], snr)
    assert float(std[0, 0, 0]) == 0.0 and float(maps["snr"][0][0, 0, 0]) == 0.0, "std == 0 -> 0, not 0 / 0"


# ------------------------------------------------------------------------------------------------ the detector
@functools.lru_cache(maxsize=None)
def score_map(name):
    rng = np.random.default_rng(7)
    if name == "one":
        s = np.array([[[0.75]]], dtype=np.float32)
    elif name == "tiny":
        s = rng.random((3, 5, 4)).astype(np.float32)
    elif name == "odd":
        s = rng.random((7, 37, 45)).astype(np.float32)
    elif name == "random":
        s = rng.standard_normal((20, 130, 197)).astype(np.float32)
    elif name == "ties":                                              # 8 levels: plateaus across tile and plane boundaries
        s = np.floor(score_map("random") * 2.0).clip(-4, 3).astype(np.float32)
    elif name == "special":
        s = rng.standard_normal((6, 40, 70)).astype(np.float32)
        flat = s.reshape(-1)
        idx = rng.permutation(flat.size)
        flat[idx[:300]] = np.nan
        flat[idx[300:330]] = np.inf
        flat[idx[330:360]] = -np.inf
        flat[idx[360:900]] = -0.0
        flat[idx[900:1400]] = 0.0
        s[0, 0, :3] = (np.nan, np.inf, np.inf)
    elif name == "flat":
        s = np.zeros((4, 20, 70), dtype=np.float32)
    s.setflags(write=False)
    return s


def check(name, thr, dist, margin=(0, 0, 0), n_max=None, capacity=1 << 20):
    from cwfa_amd import ops
    s = score_map(name)
    want = R.local_maxima(s, thr, dist, margin, n_max)
    got = ops.local_maxima(torch.tensor(s).cuda(), thr, dist, margin, n_max, capacity)
    assert got[2] == want[2], f"{name} {dist}: {got[2]} peaks, the restatement has {want[2]}"
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0]), f"{name} {dist}: positions or their order differ"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), f"{name} {dist}: scores differ"
    return got


DISTS = [(0, 0, 0), (16, 16, 16), (0, 9, 1), (5, 9, 9)]


@pytest.mark.parametrize("dist", DISTS, ids=str)
@pytest.mark.parametrize("name", ["one", "tiny", "odd", "random", "ties"])
def test_local_maxima_equal_the_restatement(name, dist):
    thr = {"one": 0.5, "tiny": 0.0, "odd": 0.3, "random": -0.5, "ties": -1.0}[name]
    zyx, sc, total = check(name, thr, dist)
    assert total >= 1 and (total > 4000 or R.far_apart(zyx, dist))
    if dist == (5, 9, 9):
        check(name, thr, dist, margin=(1, 3, 2))
        check(name, thr, dist, margin=(2, 40, 0))


@pytest.mark.parametrize("dist", DISTS, ids=str)
def test_special_values(dist):
    """NaN is never a peak and suppresses nothing; +inf peaks, ties among them to the lower index; -inf peaks only where the threshold
    lets it; -0.0 and +0.0 are one value."""
    zyx, sc, total = check("special", -np.inf, dist)
    assert total >= 1 and not np.isnan(sc).any() and sc[0] == np.inf and zyx[0].tolist() == [0, 0, 1]
    zyx0, sc0, _ = check("special", 0.0, dist)
    assert np.all(sc0 >= 0)
    if dist == (0, 0, 0):
        s = score_map("special")
        assert total == int((~np.isnan(s)).sum()) and len(sc0) == int((s >= 0).sum()) and np.signbit(sc0).any(), "-0.0 >= 0 and is returned as stored"
    check("special", np.inf, dist)
    assert check("special", np.nan, dist)[2] == 0, "nothing is >= NaN"


def test_threshold_on_a_peak_no_peaks_and_plateaus():
    zyx, sc, total = check("odd", 0.3, (2, 4, 4))
    assert total >= 3
    at = float(sc[2])
    got = check("odd", at, (2, 4, 4))
    assert got[2] == 3 and got[1][-1] == np.float32(at), "S[v] >= thr keeps the peak the threshold sits on"
    assert check("odd", float(np.nextafter(np.float32(at), np.float32(np.inf))), (2, 4, 4))[2] == 2
    assert check("odd", 2.0, (2, 4, 4))[2] == 0 and check("odd", 2.0, (2, 4, 4))[0].shape == (0, 3)
    assert check("odd", 0.3, (2, 4, 4), margin=(4, 0, 0))[2] == 0, "a margin of more than half the depth leaves nothing"
    # a constant map: a voxel leads its window only where the window's lowest index is its own -- the origin, per free axis
    assert check("flat", 0.0, (1, 9, 16))[0].tolist() == [[0, 0, 0]] and check("flat", 0.0, (16, 16, 16))[0].tolist() == [[0, 0, 0]]
    assert check("flat", 0.0, (0, 9, 16))[0].tolist() == [[z, 0, 0] for z in range(4)]
    assert check("flat", 0.0, (1, 1, 0))[0].tolist() == [[0, 0, x] for x in range(70)]
    assert check("flat", 0.0, (1, 9, 16), margin=(0, 0, 1))[2] == 0, "and inside the margin it still suppresses the rest"


def test_capacity_overflow_reruns_and_n_max_truncates():
    full = check("random", -0.5, (1, 2, 2))
    assert full[2] > 100
    small = check("random", -0.5, (1, 2, 2), capacity=4)
    assert small[2] == full[2] and np.array_equal(small[0], full[0]), "capacity 4: the second run returns the full ordered set"
    assert check("random", -0.5, (1, 2, 2), capacity=0)[2] == full[2]
    cut = check("random", -0.5, (1, 2, 2), n_max=10)
    assert cut[2] == full[2] and np.array_equal(cut[0], full[0][:10]) and np.array_equal(cut[1], full[1][:10])
    assert check("random", -0.5, (1, 2, 2), n_max=10, capacity=4)[0].shape == (10, 3)
    assert check("random", -0.5, (1, 2, 2), n_max=0)[0].shape == (0, 3)


def test_two_runs_agree_bitwise_and_the_map_is_untouched():
    from cwfa_amd import ops
    s = torch.tensor(score_map("ties")).cuda()
    keep = s.clone()
    a = ops.local_maxima(s, -1.0, (5, 9, 9))
    b = ops.local_maxima(s, -1.0, (5, 9, 9))
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert same_bits(s, keep)
    sliced = torch.tensor(score_map("random")).cuda()[:, ::2, 1:]          # a non-contiguous view is copied, not misread
    want = R.local_maxima(score_map("random")[:, ::2, 1:], 0.5, (1, 3, 3))
    got = ops.local_maxima(sliced, 0.5, (1, 3, 3))
    assert got[2] == want[2] and np.array_equal(got[0], want[0])


def test_linear_indices_past_2_to_the_31():
    """2 x 32768 x 34000 = 2.23e9 voxels: the index half of the key uses all 32 bits, and both launches walk their grid-stride loops
    (more than 2^20 tiles, more than 2^27 pixels).  Too large for the restatement; the planted answer is known: four peaks, one
    suppressed across the 2^31 boundary by a higher voxel in the other plane, one tie decided by index."""
    from cwfa_amd import ops
    D, H, W = 2, 32768, 34000
    s = torch.zeros(D, H, W, device="cuda")
    lin = lambda z, y, x: (z * H + y) * W + x
    planted = {(0, 5, 5): 1.0, (1, 31000, 100): 1.0, (1, 31000, 101): 1.0, (1, H - 1, W - 1): 1.0, (1, 32000, 500): 1.0, (0, 32000, 505): 2.0}
    for (z, y, x), v in planted.items():
        s[z, y, x] = v
    assert lin(1, 31000, 100) > 1 << 31 and lin(1, 32000, 500) > 1 << 31 > lin(0, 32000, 505) and lin(1, H - 1, W - 1) == s.numel() - 1
    zyx, sc, total = ops.local_maxima(s, 0.5, (1, 9, 9))
    assert total == 4 and zyx.tolist() == [[0, 32000, 505], [0, 5, 5], [1, 31000, 100], [1, H - 1, W - 1]] and sc.tolist() == [2.0, 1.0, 1.0, 1.0]
    zyx, sc, total = ops.local_maxima(s, 0.5, (0, 0, 0), margin=(1, 0, 0))
    assert total == 0, "two planes and a depth margin of 1 leave nothing"
    del s
    torch.cuda.empty_cache()                                           # 27 GB of map and workspace: not kept for the rest of the session


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("seed", [0, 3])
def test_planted_neurons_are_found_exactly(seed, tmp_path):
    from cwfa_amd import CWFA, ops
    st, centres = R.scene(seed)
    x = torch.tensor(st).cuda()
    am = CWFA.ActivityMap(x.shape[1:], "cuda")
    for t in range(0, x.shape[0], 8):
        am.update(x[t:t + 8])
    coords, scores = CWFA.find_neurons(am, r12=5, r3=3, thr=0.1, margin=(0, 0, 0))
    D, H, W = x.shape[1:]
    shift = D // 2 - 13
    found = sorted((z + shift, y, xx) for xx, y, z in coords)
    assert found == sorted(map(tuple, centres.tolist())), "all planted centres, nothing else"
    assert len(scores) == 24 and np.all(np.diff(scores) <= 0) and scores.min() >= 0.3
    # the same through a finished map, the default threshold (a tenth of the maximum) and the default margin
    score = am.finish("std")[0]
    c2, s2 = CWFA.find_neurons(score, margin=(0, 0, 0))
    assert c2 == coords and np.array_equal(s2, scores)
    c3, _ = CWFA.find_neurons(score)
    inner = [[int(xx), int(y), int(z) - shift] for z, y, xx in centres if 3 <= z < D - 3 and 5 <= y < H - 5 and 5 <= xx < W - 5]
    assert sorted(c3) == sorted(inner)
    assert CWFA.find_neurons(score, n_max=5, margin=(0, 0, 0))[0] == coords[:5]
    # ROIs: disjoint, around their peaks, and accepted downstream
    boxes = CWFA.roi_boxes(coords, x.shape, 5, 3)
    assert R.boxes_disjoint(boxes)
    for (xx, y, z), b in zip(coords, boxes):
        assert b[0] <= z + shift < b[1] and b[2] <= y < b[3] and b[4] <= xx < b[5]
    traces = ops.roi_means(x, boxes).cpu().numpy()
    want = np.stack([st[:, b[0]:b[1], b[2]:b[3], b[4]:b[5]].astype(np.float64).mean((1, 2, 3)) for b in boxes])
    assert traces.shape == (24, x.shape[0]) and np.allclose(traces, want, rtol=1e-12, atol=0)
    # the coordinates file
    path = str(tmp_path / "neurons.csv")
    CWFA.write_neural_coordinates_to_file(coords, path, scores)
    assert CWFA.read_neural_coordinates_from_file(path) == coords
