"""GPU: the streaming local-correlation map.  The state of cwfa_activity_update_corr_f32 against the numpy
restatement tests/corrmap_ref.py and against ops.activity_update, bit for bit, for 6, 8 and 26 neighbours, every chunking of section
22 and the smallest shapes at which the kernel can go wrong; the score against the restatement; special values; one volume larger
than a pass of the grid against a float64 torch restatement on the device; and scene with hot voxels -> ActivityMap(neighbours=26)
-> find_neurons(kind="corr") -> the restatement's peaks."""
import functools

import numpy as np
import pytest
import torch

import corrmap_ref as C
import neurons_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 7), (2, 2, 2), (3, 5, 4), (2, 3, 8), (6, 36, 44), (7, 37, 45)]
CHUNKS = [(1,) * 7, (0,) * 7, (3, 4), (7,), (1, 2, 4), "strided"]
NEIGHBOURS = [6, 8, 26]
ULP_AT_ONE = 2.0 ** -23


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def stack(shape, T=7):
    """(host, device) [T, *shape]: a mean of 100, a spread of 1, a component shared by neighbours, and one constant voxel."""
    rng = np.random.default_rng(11)
    common = rng.standard_normal((T, 1, 1, 1))
    x = (100.0 + 0.7 * common + rng.standard_normal((T, *shape))).astype(np.float32)
    x[:, 0, 0, 0] = 3.25
    x.setflags(write=False)
    return x, torch.tensor(x).cuda()


@functools.lru_cache(maxsize=None)
def reference(shape, neighbours):
    x = stack(shape)[0]
    x0, s1, s2, cc = C.accumulate(x, neighbours)
    return x0, s1, s2, cc, C.finish(s1, s2, cc, x.shape[0], neighbours)[0]


def feed(x, chunks, am):
    """The chunkings of section 22: sizes, 0 for one volume as [D,H,W], or "strided": 3 + 4 of a view whose time stride exceeds a volume."""
    if chunks == "strided":
        T, m = x.shape[0], x[0].numel()
        wide = torch.zeros(T, m + 8, device="cuda")
        wide[:, :m] = x.reshape(T, m)
        view = wide.as_strided(tuple(x.shape), (m + 8, x.shape[2] * x.shape[3], x.shape[3], 1))
        assert view.stride(0) == m + 8 and torch.equal(view, x)
        x, chunks = view, (3, 4)
    t = 0
    for c in chunks:
        am.update(x[t] if c == 0 else x[t:t + c])
        t += max(c, 1)
    assert t == x.shape[0] and am.count == t
    return am


@functools.lru_cache(maxsize=None)
def plain_state(shape, chunks):
    from cwfa_amd.CWFA import ActivityMap
    return feed(stack(shape)[1], chunks, ActivityMap(shape, "cuda")).state


@functools.lru_cache(maxsize=None)
def one_chunk_score(shape, neighbours):
    from cwfa_amd.CWFA import ActivityMap
    return feed(stack(shape)[1], (7,), ActivityMap(shape, "cuda", neighbours=neighbours)).finish("corr")[0]


# ------------------------------------------------------------------------------------------------ the state and the score
@pytest.mark.parametrize("chunks", CHUNKS, ids=str)
@pytest.mark.parametrize("neighbours", NEIGHBOURS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_state_is_the_restatement_and_the_plain_kernel_bit_for_bit(shape, neighbours, chunks):
    from cwfa_amd.CWFA import ActivityMap
    x0, s1, s2, cc, score = reference(shape, neighbours)
    am = feed(stack(shape)[1], chunks, ActivityMap(shape, "cuda", neighbours=neighbours))
    assert same_bits(am.state[0], x0) and same_bits(am.state[1], s1) and same_bits(am.state[2], s2), "x0 / s1 / s2 differ from the restatement"
    got = am.cc.cpu().numpy()
    assert got.shape == cc.shape and same_bits(got, cc), "cc differs from the restatement"
    for k, o in enumerate(C.forward(neighbours)):
        outside = np.ones(shape, dtype=bool)
        outside[C.pair(shape, o)[0][1:]] = False
        assert not bits(got[k])[outside].any(), f"cc[{k}] is not +0.0 where the neighbour {o} is outside the volume"
    for a, b in zip(am.state, plain_state(shape, chunks)):
        assert same_bits(a, b), "the state differs from what ops.activity_update writes for the same chunks"
    # the score: both sides evaluate the same float64 expressions (IEEE division and square root on either side) from the same
    # state, so it is held to the restatement's bits, which is what it came out as; the bound derived beforehand was one fp32 ulp at 1
    sc, mean, std, vmax, vmin = am.finish("corr")
    worst = float(np.abs(sc.cpu().numpy().astype(np.float64) - score.astype(np.float64)).max())
    print(f"{shape} {neighbours} {chunks}: score differs from the restatement by at most {worst:.3g}; bitwise equal: {same_bits(sc, score)}")
    assert not bool(torch.isnan(sc).any()) and worst <= ULP_AT_ONE and same_bits(sc, score)
    assert same_bits(sc, one_chunk_score(shape, neighbours)), "the score depends on the chunking"
    assert same_bits(am.finish("corr")[0], sc), "two runs differ"
    assert float(sc[0, 0, 0]) == 0.0, "the constant voxel"
    # the other kinds on this object are the plain object's
    plain = ActivityMap(shape, "cuda")
    plain.state, plain.count = plain_state(shape, chunks), 7
    assert all(same_bits(a, b) for a, b in zip(am.finish("snr"), plain.finish("snr")))
    assert same_bits(mean, plain.finish("std")[1]) and same_bits(std, plain.finish("std")[2])


@pytest.mark.parametrize("neighbours", NEIGHBOURS)
def test_special_values(neighbours):
    """The CPU cases on the device: a constant voxel, NaN, +inf, -inf, +inf as the first sample, N = 1."""
    from cwfa_amd.CWFA import ActivityMap
    x, y, planted = C.special_stack()
    run = lambda a, chunks: feed(torch.tensor(a).cuda(), chunks, ActivityMap(a.shape[1:], "cuda", neighbours=neighbours))
    clean, sc = run(x, (2, 4)).finish("corr")[0], run(y, (2, 4)).finish("corr")[0]
    assert not bool(torch.isnan(sc).any()) and not bool(torch.isnan(clean).any())
    for got, src in ((clean, x), (sc, y)):
        assert float(np.abs(got.cpu().numpy().astype(np.float64) - C.score(src, neighbours).astype(np.float64)).max()) <= ULP_AT_ONE
    touched = C.touched(planted, x.shape[1:], neighbours)
    assert np.array_equal(bits(sc)[~touched], bits(clean)[~touched]), "more than the voxels and their neighbours changed"
    assert float(sc[1, 1, 1]) == 0.0, "a constant voxel scores 0"
    # a NaN in one series: no NaN in the map, and only that voxel's and its neighbours' scores change
    z = x.copy()
    z[3, 1, 3, 4] = np.nan
    one = run(z, (1, 5)).finish("corr")[0]
    near = C.touched([(1, 3, 4)], x.shape[1:], neighbours)
    assert not bool(torch.isnan(one).any()) and np.array_equal(bits(one)[~near], bits(clean)[~near])
    assert (bits(one)[near] != bits(clean)[near]).all()
    first = run(x[:1], (1,))
    assert not bool(first.finish("corr")[0].any()) and not bool(first.cc.any()), "N = 1: every pair has den = 0"


# ------------------------------------------------------------------------------------------------ more voxels than one pass of the grid
def test_grid_stride_takes_two_steps():
    """9 x 1024 x 1024 voxels: more than the 8192 blocks x 256 threads x 4 voxels of one pass of the update kernel's grid (and than the
    16384 x 256 of the finish kernel's).  T = 3 as 1 + 2, 6 neighbours, against sequential float64 torch operators on the device."""
    from cwfa_amd.CWFA import ActivityMap
    shape = (9, 1024, 1024)
    assert shape[0] * shape[1] * shape[2] > 8192 * 256 * 4
    g = torch.Generator(device="cuda").manual_seed(2)
    x = 10.0 + torch.randn(3, *shape, device="cuda", generator=g)
    am = ActivityMap(shape, "cuda", neighbours=6).update(x[:1]).update(x[1:])
    fw = C.forward(6)
    x0 = x[0].double()
    s1, s2 = torch.zeros_like(x0), torch.zeros_like(x0)
    cc = torch.zeros(3, *shape, dtype=torch.float64, device="cuda")
    for t in (1, 2):
        d = x[t].double().sub(x0)
        s1 = s1.add(d)
        s2 = s2.add(d.mul(d))
        for k, o in enumerate(fw):
            lo, hi = C.pair(shape, o)
            cc[k][lo] = cc[k][lo].add(d[lo].mul(d[hi]))
    as_int = lambda t: t.view(torch.int64)
    assert torch.equal(as_int(am.state[1]), as_int(s1)) and torch.equal(as_int(am.state[2]), as_int(s2))
    assert torch.equal(as_int(am.cc), as_int(cc)) and torch.equal(am.state[0], x[0])
    assert torch.equal(am.state[3], x.amax(0)) and torch.equal(am.state[4], x.amin(0))
    # the finish kernel, by the same expressions
    v = s2.sub(s1.mul(s1).div(3.0)).clamp_min(0.0)
    total, n = torch.zeros_like(s1), torch.zeros_like(s1)
    for o in C.offsets(6):
        lo, hi = C.pair(shape, o)
        c = cc[fw.index(o)][lo] if o > (0, 0, 0) else cc[fw.index(tuple(-a for a in o))][hi]
        cov = c.sub(s1[lo].mul(s1[hi]).div(3.0))
        den = v[lo].mul(v[hi]).sqrt()
        total[lo] = total[lo].add(torch.where(den > 0.0, cov.div(den), torch.zeros_like(den)))
        n[lo] += 1.0
    want = total.div(n).float()
    sc = am.finish("corr")[0]
    worst = float((sc.double() - want.double()).abs().max())
    print(f"grid-stride: score differs from the torch restatement by at most {worst:.3g}")
    assert worst <= ULP_AT_ONE and float(sc.abs().max()) <= 1.0
    del x, cc, am
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("seed", [0, 1])
def test_neurons_among_hot_voxels_are_found_exactly(seed):
    from cwfa_amd import CWFA, ops
    st, centres = C.scene_hot(seed)
    zyx, scores, total = C.scene_peaks(seed)
    x = torch.tensor(st).cuda()
    am = CWFA.ActivityMap(x.shape[1:], "cuda", neighbours=26)
    for t in range(0, x.shape[0], 8):
        am.update(x[t:t + 8])
    coords, sc = CWFA.find_neurons(am, r12=5, r3=3, thr=C.THR, margin=C.MARGIN, dist=C.DIST, kind="corr")
    shift = x.shape[1] // 2 - 13
    found = [(z + shift, y, xx) for xx, y, z in coords]
    assert total == len(centres) == 24 and sorted(found) == sorted(map(tuple, zyx.tolist())), "the restatement's peaks, nothing else"
    order = {p: i for i, p in enumerate(map(tuple, zyx.tolist()))}
    assert float(np.abs(sc.astype(np.float64) - scores[[order[p] for p in found]].astype(np.float64)).max()) <= ULP_AT_ONE
    boxes = CWFA.roi_boxes(coords, x.shape, 5, 3)
    assert R.boxes_disjoint(boxes)
    # the std map of the same object still takes hot voxels for neurons
    assert len(CWFA.find_neurons(am, r12=5, r3=3, rel_thr=0.1, margin=C.MARGIN, dist=C.DIST)[0]) > 24
    mean, std = ops.stack_mean_std(x)
    _, mo, so, _, _ = am.finish("corr")
    assert same_bits(mo, mean) and same_bits(so, std), "mean / std differ from stack_mean_std of the whole stack"
