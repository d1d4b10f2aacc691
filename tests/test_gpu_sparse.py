"""GPU: sparse-activity extraction, bit for bit against the numpy restatement tests/sparse_ref.py at the smallest
shapes that reach every path: both forms of the per-pixel selection across the wave-split remainders, the tile edges and the form
switch; the float64 frame dots (exact on integer data, inside the any-order bound on random data, bitwise repeatable, additive over
bands); the residual in all its layouts; ``extract_sparse`` end to end on an integer scene, and the dataset on top of it."""
import functools
import math

import numpy as np
import pytest
import torch

import sparse_ref as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": (np.float32, torch.float32), "fp16": (np.float16, torch.float16)}


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def tt(x):
    """A numpy array (possibly read-only) as a torch tensor of its own."""
    return torch.from_numpy(np.array(x))


def device_stack(x, stride_pad=0, offset=0):
    """x [T, P] (numpy) on the device as a [T, P] view with ``stride_pad`` unused elements behind every frame, starting ``offset``
    elements into its buffer; the gaps hold a large value no selection may see."""
    T, P = x.shape
    fs = P + stride_pad
    buf = torch.full((offset + T * fs,), 3e4, dtype=tt(x[:1]).dtype, device="cuda")
    view = buf.as_strided((T, P), (fs, 1), offset)
    view.copy_(tt(x))
    assert view.data_ptr() == buf.data_ptr() + offset * buf.element_size() and (T < 2 or view.stride(0) == fs)
    return view


@functools.lru_cache(maxsize=None)
def data(kind, T, P, dt, seed=0):
    """[T, P] numpy data of one kind, every value finite in ``dt``."""
    rng = np.random.default_rng(seed + 1000 * T + P)
    npdt = DTYPES[dt][0]
    big = 6e4 if dt == "fp16" else 3e38
    if kind == "equal":
        x = np.full((T, P), 2.5)
    elif kind == "grid":
        x = rng.choice([-1.0, 0.0, 0.5, 7.0], size=(T, P))
    elif kind == "zeros":
        x = rng.choice([-3.0, -0.0, 0.0, 0.0, -0.0, 1e-3, 2.0], size=(T, P))
    elif kind == "subnormal":
        x = rng.integers(-40, 40, size=(T, P)) * 5.960464477539063e-08               # multiples of the smallest fp16 subnormal
    elif kind == "large":
        x = rng.choice([-big, -big / 2, -1.0, 1.0, big / 2, big], size=(T, P))
    else:                                                                              # mixed: many magnitudes, ties, both zeros
        x = rng.standard_normal((T, P)) * 10.0 ** rng.integers(-3, 4, size=(T, P))
        x[rng.random((T, P)) < 0.1] = 0.0
        x[rng.random((T, P)) < 0.1] = -0.0
        x[rng.random((T, P)) < 0.2] = 1.25
    x = x.astype(npdt)
    assert np.isfinite(x).all()
    x.setflags(write=False)
    return x


def background(T, P, seed=0):
    rng = np.random.default_rng(seed + 7)
    return (0.5 + rng.random(T)).astype(np.float32), (rng.standard_normal(P) * 3).astype(np.float32)


def run_select(x, ranks, ab=None, forms=("lds", "stream", "auto"), **view):
    """Every requested form on the device against the restatement; returns the results by form."""
    from cwfa_amd import ops
    xd = device_stack(x, **view)
    a = b = None
    if ab is not None:
        a, b = (tt(v).cuda() for v in ab)
    ref = R.select(x, ranks, *(ab or ()))
    got = {}
    for form in forms:
        out = ops.temporal_select(xd, ranks, a=a, b=b, form=form)
        assert out.shape == (len(ranks), x.shape[1]) and out.dtype == torch.float32
        assert same_bits(out, ref), f"form {form}: differs from the restatement"
        got[form] = out
    return got


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("transformed", [False, True], ids=["plain", "background"])
@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("T", [1, 2, 3, 63, 64, 65, 250, "cap", "cap+1"], ids=str)
def test_select_over_the_frame_counts(T, dt, transformed):
    """The wave-split remainders (T around one and around eight waves' rows), the reference's 250 frames, and the boundary of the
    one-read form, read from the library: at cap both forms run, at cap + 1 the one-read form refuses and auto streams."""
    from cwfa_amd import _lib, ops
    cap = ops.temporal_lds_frames(DTYPES[dt][1], transformed)
    T = cap if T == "cap" else cap + 1 if T == "cap+1" else T
    P = 130
    x = data("mixed", T, P, dt)
    ranks = [0, T - 1, T // 2, T // 2]
    ab = background(T, P) if transformed else None
    if T <= cap:
        run_select(x, ranks, ab)
    else:
        run_select(x, ranks, ab, forms=("stream", "auto"))
        with pytest.raises(_lib.CwfaHipError, match="one-read form"):
            a, b = (tt(v).cuda() for v in ab) if transformed else (None, None)
            ops.temporal_select(device_stack(x), ranks, a=a, b=b, form="lds")


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_select_over_the_tile_edges_strides_and_ranks(P, dt):
    """One tile, one tile exactly, one pixel into the second, three tiles; a frame stride above P and a base one element into the
    buffer (an odd fp16 address); K = 1 .. 4 with the extreme ranks, the middle and a duplicate."""
    T = 65
    x = data("mixed", T, P, dt)
    for ranks in ([T // 2], [0, T - 1], [T - 1, 0, 31], [5, 64, 5, 0]):
        run_select(x, ranks, forms=("lds", "stream"), stride_pad=3, offset=1)
    run_select(x, [0, 32, 32, 64], background(T, P), forms=("lds", "stream"), stride_pad=5, offset=1)


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("kind", ["equal", "grid", "zeros", "subnormal", "large"])
def test_select_on_hard_data(kind, dt):
    T, P = 64, 65
    x = data(kind, T, P, dt)
    got = run_select(x, [0, 20, 43, 63], forms=("lds", "stream"))
    if kind == "zeros":
        z = bits(got["lds"])
        assert not np.any(z == 0x80000000), "a zero comes back as +0"
    if kind == "equal":
        assert float(got["lds"].min()) == float(got["lds"].max()) == 2.5
    run_select(x, [0, 31, 63], background(T, P), forms=("lds", "stream"))


def test_select_of_a_three_dimensional_stack_and_a_band_of_rows():
    from cwfa_amd import ops
    x = data("mixed", 9, 6 * 10, "fp32").reshape(9, 6, 10)
    xd = tt(x).cuda()
    out = ops.temporal_select(xd, [4])
    assert out.shape == (1, 6, 10) and same_bits(out.reshape(1, -1), R.select(x, [4]))
    band = ops.temporal_select(xd[:, 2:5], [0, 8])
    assert same_bits(band.reshape(2, -1), R.select(np.ascontiguousarray(x[:, 2:5]), [0, 8]))
    with pytest.raises(ValueError, match="ranks"):
        ops.temporal_select(xd, [9])
    with pytest.raises(ValueError, match="1 to 4"):
        ops.temporal_select(xd, [0] * 5)
    with pytest.raises(ValueError, match="together"):
        ops.temporal_select(xd, [0], a=torch.ones(9, device="cuda"))


# ------------------------------------------------------------------------------------------------ frame dots
def int_stack(T, P, dt, seed=0):
    rng = np.random.default_rng(seed + T + P)
    return rng.integers(0, 1000, size=(T, P)).astype(DTYPES[dt][0]), rng.integers(0, 1000, size=P).astype(np.float32)


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("T,P,view", [(5, 1, {}), (7, 1023, {}), (3, 1024, {}), (9, 1028, {}), (4, 5001, {}), (3, 8200, {}),
                                      (600, 8, {}), (6, 1028, dict(stride_pad=4)), (6, 1028, dict(stride_pad=3)),
                                      (6, 1028, dict(offset=1))], ids=str)
def test_frame_dots_are_exact_on_integers(T, P, view, dt):
    """Integers below 1000: every product and every partial sum is an integer below 2^53, exact in any order -- one slab, its last
    pixel, two waves, two blocks, more frames than a block's chunk; 16-byte loads and element loads (odd P, odd stride, odd base)."""
    from cwfa_amd import ops
    x, b = int_stack(T, P, dt)
    ref = R.frame_dots(x, b)
    assert float(ref.max()) < 2.0 ** 53
    got = ops.frame_dots(device_stack(x, **view), tt(b).cuda())
    assert got.dtype == torch.float64 and got.shape == (T + 1,) and same_bits(got, ref)


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_frame_dots_on_random_data_stay_inside_the_any_order_bound_and_repeat(dt):
    from cwfa_amd import ops
    T, P = 11, 4999
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((T, P)) * 100).astype(DTYPES[dt][0])
    b = (rng.standard_normal(P) * 100).astype(np.float32)
    xd, bd = tt(x).cuda(), tt(b).cuda()
    got = ops.frame_dots(xd, bd)
    terms = np.concatenate([x.astype(np.float64) * b.astype(np.float64)[None], (b.astype(np.float64) ** 2)[None]])
    exact = np.array([math.fsum(row.tolist()) for row in terms])                # the correctly rounded sums of the exact products
    bound = P * 2.0 ** -53 * np.abs(terms).sum(axis=1)                     # the products are exact; any order of P additions
    err = np.abs(got.cpu().numpy() - exact)
    print("frame_dots: largest error / bound =", float((err / bound).max()))
    assert np.all(err <= bound)
    assert same_bits(ops.frame_dots(xd, bd), got), "bitwise repeatable"


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_frame_dots_of_two_bands_add_up_to_the_whole(dt):
    from cwfa_amd import ops
    T, H, W = 5, 37, 36
    x, b = int_stack(T, H * W, dt)
    xd, bd = tt(x).cuda().reshape(T, H, W), tt(b).cuda().reshape(H, W)
    whole = ops.frame_dots(xd, bd)
    sums = ops.frame_dots(xd[:, :17], bd[:17])
    assert ops.frame_dots(xd[:, 17:], bd[17:], sums=sums) is sums
    assert same_bits(sums, whole) and same_bits(whole, R.frame_dots(x, b))
    zero = ops.frame_dots(xd, torch.zeros_like(bd))
    assert same_bits(zero, np.zeros(T + 1)), "an all-zero baseline"
    with pytest.raises(ValueError, match="sums"):
        ops.frame_dots(xd, bd, sums=torch.zeros(T, dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------------------------------------ the residual
@pytest.mark.parametrize("pair", [False, True], ids=["map", "pair"])
@pytest.mark.parametrize("with_tau", [True, False], ids=["tau", "no_tau"])
@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("T,P,view", [(20, 1028, {}), (3, 1031, {}), (3, 1028, dict(offset=1)), (3, 1028, dict(stride_pad=2)), (1, 1, {})],
                         ids=["vector", "odd_P", "odd_base", "odd_stride", "one"])
def test_residual_is_the_restatement(T, P, view, dt, with_tau, pair):
    from cwfa_amd import ops
    x = data("mixed", T, P, dt)
    a, b = background(T, P)
    tau = np.abs(background(T, P, seed=3)[1]) if with_tau else None
    ref = R.residual(x, a, b, tau, pair)
    dev = lambda v: None if v is None else tt(v).cuda()
    got = ops.sparse_residual(device_stack(x, **view), dev(a), dev(b), dev(tau), pair=pair)
    assert got.shape == ref.shape and same_bits(got, ref)
    assert float(got[..., 1].min() if pair else got.min()) >= 0.0
    out = torch.empty_like(got)
    assert ops.sparse_residual(device_stack(x, **view), dev(a), dev(b), dev(tau), out=out, pair=pair) is out and same_bits(out, ref)


@pytest.mark.parametrize("P", [1028, 1031])
def test_residual_in_place(P):
    from cwfa_amd import ops
    T = 6
    x = data("mixed", T, P, "fp32")
    a, b = background(T, P)
    xd = tt(x.copy()).cuda()
    assert ops.sparse_residual(xd, tt(a).cuda(), tt(b).cuda(), out=xd) is xd
    assert same_bits(xd, R.residual(x, a, b))
    with pytest.raises(ValueError, match="out must be"):
        ops.sparse_residual(xd, tt(a).cuda(), tt(b).cuda(), out=xd, pair=True)


# ------------------------------------------------------------------------------------------------ extract_sparse and the dataset
def check_split(got, ref):
    assert same_bits(got.baseline, ref.baseline), "baseline"
    assert same_bits(got.scales, ref.scales), "scales"
    assert (got.tau is None) == (ref.tau is None) and (ref.tau is None or same_bits(got.tau, ref.tau)), "tau"
    assert got.sparse.shape == ref.sparse.shape and same_bits(got.sparse, ref.sparse), "sparse"


@pytest.mark.parametrize("pair", [False, True], ids=["map", "pair"])
@pytest.mark.parametrize("scale", ["ls", "none"])
@pytest.mark.parametrize("noise_k", [0, 3])
@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_extract_sparse_is_determined_on_an_integer_scene(dt, noise_k, scale, pair):
    """Integer frames give integer sums, exact in any order: every field of the result is fixed, and equals the restatement's."""
    from cwfa_amd.XLFMDataset import SparseSplit, extract_sparse
    x = R.grid_scene(0, dtype=DTYPES[dt][0])
    kw = dict(baseline_q=0.3, noise_k=noise_k, ths=0.5 if noise_k else 0.0, scale=scale, pair=pair)
    got = extract_sparse(tt(x).cuda(), **kw)
    assert isinstance(got, SparseSplit) and got._fields == ("sparse", "baseline", "scales", "tau")
    check_split(got, R.extract_sparse(x, **kw))
    assert float(got.sparse[..., 1].max() if pair else got.sparse.max()) > 20.0, "the planted transients are there"
    if scale == "ls":
        assert float(got.scales[0]) > float(got.scales[-1]), "the fade is in the scales"


def test_extract_sparse_thresholds_and_a_dead_stack():
    from cwfa_amd.XLFMDataset import extract_sparse
    x = R.grid_scene(1)
    xd = tt(x).cuda()
    check_split(extract_sparse(xd, ths=2.0), R.extract_sparse(x, ths=2.0))              # ths alone: a constant map
    dead = extract_sparse(torch.zeros(5, 4, 6, device="cuda"))
    assert same_bits(dead.scales, np.zeros(5, dtype=np.float32)) and float(dead.sparse.abs().max()) == 0.0, "0 / 0 gives scales of 0"
    work = xd.clone()
    assert extract_sparse(work, out=work).sparse is work and same_bits(work, R.extract_sparse(x).sparse), "in place"


def test_from_tensors_sparse_is_prepare_frames_then_extract_sparse():
    from cwfa_amd.XLFMDataset import XLFMDatasetFull, extract_sparse, prepare_frames
    raw = tt(R.grid_scene(2, T=12, H=14, W=14)).cuda()
    vols = torch.zeros(12, 2, 4, 4, dtype=torch.float16, device="cuda")
    frames = prepare_frames(raw, (8, 12))
    plain = XLFMDatasetFull.from_tensors(raw, vols, (8, 12))
    assert same_bits(plain.stacked_views, frames), "sparse=None: unchanged"
    ds = XLFMDatasetFull.from_tensors(raw, vols, (8, 12), sparse=True)
    assert ds.stacked_views.shape == (12, 8, 12) and same_bits(ds.stacked_views, extract_sparse(frames).sparse)
    kw = dict(noise_k=2.0, baseline_q=0.3, pair=True)
    ds = XLFMDatasetFull.from_tensors(raw, vols, (8, 12), "set", sparse=kw)
    assert ds.dataset_id == "set" and ds.stacked_views.shape == (12, 8, 12, 2)
    assert same_bits(ds.stacked_views, extract_sparse(frames, **kw).sparse) and same_bits(ds.stacked_views[..., 0], frames)
    assert same_bits(ds.stacked_views, R.extract_sparse(frames.cpu().numpy(), **kw).sparse)


def test_statistics_of_the_pair_layout_are_those_of_its_channels():
    from cwfa_amd import ops
    from cwfa_amd.XLFMDataset import ConcatDataset, XLFMDatasetFull
    sets = []
    for seed, T in ((3, 12), (4, 9)):
        raw = tt(R.grid_scene(seed, T=T, H=14, W=14)).cuda()
        vols = tt(np.random.default_rng(seed).random((T, 2, 4, 4)).astype(np.float16)).cuda()
        sets.append(XLFMDatasetFull.from_tensors(raw, vols, (8, 12), sparse=dict(pair=True, noise_k=1.0)))
    stats = ConcatDataset(*sets).get_statistics()
    c0 = ops.mean_std([d.stacked_views[..., 0].contiguous() for d in sets])
    c1 = ops.mean_std([d.stacked_views[..., 1].contiguous() for d in sets])
    want = [torch.tensor(v, dtype=torch.float64).to(torch.float32) for v in (c0[0], c0[1], c1[0], c1[1])]
    assert len(stats) == 6 and all(same_bits(s, w) for s, w in zip(stats[:4], want))
    assert float(stats[0]) > float(stats[2]) > 0.0, "the sparse channel is the smaller one"
