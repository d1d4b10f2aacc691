"""CPU: sparse-activity extraction without a GPU -- the numpy restatement tests/sparse_ref.py checked against
itself (keys, sort against bisection), the rank rule against numpy.quantile, the model on the planted scene, the argument validation
of the new entry points through the built library, and the refusals the Python layer decides before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_ref as R


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


def ranks_arg(*r):
    return (ctypes.c_int * len(r))(*r)


# ------------------------------------------------------------------------------------------------ the restatement
def test_keys_order_like_the_values_and_invert():
    v = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, 65504.0, 3e38, np.inf], dtype=np.float32)
    k = R.key32(v).astype(np.int64)
    assert k[3] == k[4], "-0 and +0 are one value"
    assert np.all(np.diff(np.delete(k, 3)) > 0)
    back = R.unkey32(R.key32(v))
    assert np.array_equal(np.delete(back, 3).view(np.uint32), np.delete(v, 3).view(np.uint32)) and back[3].view(np.uint32) == 0
    h = np.array([-65504.0, -1.0, -6e-8, -0.0, 0.0, 6e-8, 6.1e-5, 1.0, 65504.0], dtype=np.float16)      # 6e-8: the subnormal
    k16 = R.key16(h).astype(np.int64)
    assert k16[3] == k16[4] and np.all(np.diff(np.delete(k16, 3)) > 0)
    assert np.array_equal(np.delete(R.unkey16(R.key16(h)), 3).view(np.uint16), np.delete(h, 3).view(np.uint16))
    # every fp16 bit pattern that is finite: 16-bit keys order like the 32-bit keys of the widened values
    allh = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    allh = allh[np.isfinite(allh)]
    assert np.array_equal(np.argsort(R.key16(allh), kind="stable"), np.argsort(R.key32(allh.astype(np.float32)), kind="stable"))


@pytest.mark.parametrize("T", [1, 2, 7, 64, 65])
def test_bisection_is_the_sort(T):
    rng = np.random.default_rng(T)
    grid = rng.choice(np.array([-2.5, -0.0, 0.0, 1.0, 7.0], dtype=np.float32), size=(T, 33))                 # heavy ties, both zeros
    wide = (rng.standard_normal((T, 33)) * 10.0 ** rng.integers(-30, 30, size=(T, 33))).astype(np.float32)
    ranks = sorted({0, T // 2, T - 1})
    for x in (grid, wide):
        k = R.key32(x)
        assert np.array_equal(R.select_bisect(k, ranks, 32), R.select_sort(k, ranks).astype(np.uint64))
        got = R.select(x, ranks)
        assert np.array_equal(got, np.sort(x + np.float32(0), axis=0)[ranks]), "the value is the sorted element"
    h = grid.astype(np.float16)
    assert np.array_equal(R.select_bisect(R.key16(h), ranks, 16), R.select_sort(R.key16(h), ranks).astype(np.uint64))
    assert np.array_equal(R.select(h, ranks), R.select(h.astype(np.float32), ranks)), "16-bit and 32-bit keys select the same value"


def test_selection_with_a_background_orders_the_residual():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 50, size=(9, 20)).astype(np.float32)
    a, b = rng.random(9).astype(np.float32), rng.integers(0, 40, size=20).astype(np.float32)
    v = x - (a[:, None] * b[None, :]).astype(np.float32)
    assert np.array_equal(R.select(x, [0, 4, 8], a, b), np.sort(v + np.float32(0), axis=0)[[0, 4, 8]])
    assert np.array_equal(R.residual(x, a, b), np.maximum(v, 0))
    assert np.array_equal(R.residual(x, a, b, pair=True)[..., 0], x)


@pytest.mark.parametrize("q", [0.0, 0.1, 0.1587, 0.25, 0.3, 0.5, 0.7, 0.9, 0.99, 1.0])
@pytest.mark.parametrize("n", [1, 2, 3, 10, 11, 64, 120, 250, 251, 1000])
def test_rank_rule_is_numpy_quantile_lower(q, n):
    from cwfa_amd.XLFMDataset import quantile_rank
    x = np.arange(n, dtype=np.float64)                                     # the value IS the rank
    assert quantile_rank(q, n) == R.quantile_rank(q, n) == int(np.quantile(x, q, method="lower"))


def test_rank_rule_refuses_nonsense():
    from cwfa_amd.XLFMDataset import quantile_rank
    for q, n in ((-0.1, 5), (1.5, 5), (0.5, 0), (float("nan"), 5)):
        with pytest.raises(ValueError, match="quantile"):
            quantile_rank(q, n)


# ------------------------------------------------------------------------------------------------ the model on the planted scene
@pytest.fixture(scope="module")
def planted():
    sc = R.scene(0)
    return sc, {k: R.extract_sparse(sc.frames, noise_k=k) for k in (0, 1, 2, 3)}


def test_scales_follow_the_planted_bleaching(planted):
    sc, res = planted
    corr = float(np.corrcoef(res[0].scales.astype(np.float64), sc.bleach)[0, 1])
    print(f"corr(scales, bleaching) = {corr:.5f}")
    assert corr >= 0.99
    assert res[0].tau is None and res[3].tau is not None


def test_off_support_fraction_falls_with_the_threshold(planted):
    sc, res = planted
    off = ~sc.support
    frac = [float((res[k].sparse[:, off] > 0).mean()) for k in (0, 1, 2, 3)]
    print("off-support non-zero fraction at k = 0, 1, 2, 3:", [f"{f:.4f}" for f in frac])
    assert all(a > b for a, b in zip(frac, frac[1:])), frac
    assert 0.3 < frac[0] < 0.7, "without a threshold about half of the noise is positive"


def test_rank1_background_leaks_less_than_a_static_one(planted):
    sc, res = planted
    off = ~sc.support
    static = R.extract_sparse(sc.frames, scale="none")
    leak = lambda r: float(r.sparse[:, off].mean())
    print(f"mean off-support residual: static baseline {leak(static):.2f}, rank-1 {leak(res[0]):.2f}")
    assert leak(res[0]) < 0.6 * leak(static)
    assert np.array_equal(static.scales, np.ones(sc.frames.shape[0], dtype=np.float32))


def test_grid_scene_sums_are_exact_integers():
    for dt in (np.float32, np.float16):
        x = R.grid_scene(0, dtype=dt)
        assert np.array_equal(x, np.round(x)) and float(x.max()) < 2048, "exact in fp16"
        b = R.select(x, [R.quantile_rank(0.5, x.shape[0])])[0]
        s = R.frame_dots(x, b)
        assert np.array_equal(s, np.round(s)) and float(s.max()) < 2.0 ** 53
        assert float(b.reshape(x.shape[1:])[0, 0]) == 0.0, "the dead pixel"


# ------------------------------------------------------------------------------------------------ the entry points' arguments
def test_temporal_select_arguments(L, ptr):
    q = [ctypes.c_void_p(ptr.value + 2048 * k) for k in range(4)]
    x, a, b, out = q
    r1 = ranks_arg(1)

    def call(x=x, dtype=0, T=4, P=8, fs=8, a=None, b=None, ranks=r1, K=1, out=out, form=0):
        return L.cwfa_temporal_select(x, dtype, T, P, fs, a, b, ranks, K, out, form, None)

    assert call(x=None) == -1 and call(ranks=None) == -1 and call(out=None) == -1
    assert b"cwfa_temporal_select: null" in L.cwfa_last_error()
    assert call(dtype=2) == -1 and call(dtype=-1) == -1 and b"dtype" in L.cwfa_last_error()
    assert call(T=-1) == -2 and call(P=-8) == -2 and b"negative" in L.cwfa_last_error()
    assert call(fs=7) == -1 and b"stride" in L.cwfa_last_error()
    for K in (0, 5, -1):
        assert call(K=K, ranks=ranks_arg(0, 0, 0, 0, 0)) == -1 and b"1 .. 4" in L.cwfa_last_error()
    assert call(ranks=ranks_arg(4)) == -1 and call(ranks=ranks_arg(-1)) == -1 and b"rank" in L.cwfa_last_error()
    assert call(ranks=ranks_arg(0, 3, 4), K=3) == -1, "every rank is checked"
    assert call(a=a) == -1 and call(b=b) == -1 and b"together" in L.cwfa_last_error()
    assert call(form=3) == -1 and call(form=-1) == -1 and b"form" in L.cwfa_last_error()
    for dtype, tr in ((0, 0), (0, 1), (1, 0), (1, 1)):
        cap = L.cwfa_temporal_select_lds_frames(dtype, tr)
        assert cap >= 250, "the one-read form holds the reference's 250-frame stacks"
        kw = dict(dtype=dtype, T=cap + 1, a=a if tr else None, b=b if tr else None, form=1)
        assert call(**kw) == -2 and b"one-read form" in L.cwfa_last_error(), (dtype, tr)
    assert L.cwfa_temporal_select_lds_frames(1, 0) == 2 * L.cwfa_temporal_select_lds_frames(0, 0), "16-bit keys: twice the frames"
    assert L.cwfa_temporal_select_lds_frames(1, 1) == L.cwfa_temporal_select_lds_frames(0, 1) == L.cwfa_temporal_select_lds_frames(0, 0)
    assert L.cwfa_temporal_select_lds_frames(2, 0) == -1
    assert call(T=0, ranks=ranks_arg(0)) == 0 and call(P=0, fs=0) == 0, "empty: no launch"


def test_frame_dots_arguments(L, ptr):
    x, b, sums, ws = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(4))

    def call(x=x, dtype=0, T=4, P=8, fs=8, b=b, sums=sums, ws=ws, acc=0):
        return L.cwfa_frame_dots(x, dtype, T, P, fs, b, sums, ws, acc, None)

    assert call(x=None) == -1 and call(b=None) == -1 and call(sums=None) == -1 and call(ws=None) == -1
    assert b"cwfa_frame_dots: null" in L.cwfa_last_error()
    assert call(dtype=3) == -1 and call(acc=2) == -1
    assert call(T=-1) == -2 and call(P=-1) == -2
    assert call(fs=7) == -1 and b"stride" in L.cwfa_last_error()
    assert call(sums=ctypes.c_void_p(sums.value + 4)) == -3 and b"8-byte" in L.cwfa_last_error()
    assert call(ws=ctypes.c_void_p(ws.value + 4)) == -3
    assert call(P=0, fs=0, acc=1) == 0, "empty and accumulating: nothing to do"
    assert L.cwfa_frame_dots_workspace_bytes(4, 0) == 0 and L.cwfa_frame_dots_workspace_bytes(-1, 8) == -1
    assert L.cwfa_frame_dots_workspace_bytes(4, 8) >= 5 * 8 and L.cwfa_frame_dots_workspace_bytes(4, 8) % 8 == 0
    big = L.cwfa_frame_dots_workspace_bytes(250, 2160 * 2160)
    assert big % (251 * 8) == 0 and big <= 8 << 20, "a few MiB at the reference's stack"


def test_sparse_residual_arguments(L, ptr):
    x, a, b, tau, out = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(5))

    def call(x=x, dtype=0, T=4, P=8, fs=8, a=a, b=b, tau=tau, out=out, pair=0):
        return L.cwfa_sparse_residual(x, dtype, T, P, fs, a, b, tau, out, pair, None)

    for k in ("x", "a", "b", "out"):
        assert call(**{k: None}) == -1 and b"cwfa_sparse_residual: null" in L.cwfa_last_error()
    assert call(dtype=2) == -1 and call(pair=2) == -1
    assert call(T=-1) == -2 and call(P=-1) == -2
    assert call(fs=7) == -1 and b"stride" in L.cwfa_last_error()
    for kw in (dict(pair=1), dict(dtype=1), dict(fs=9)):
        assert call(out=x, **kw) == -1 and b"in place" in L.cwfa_last_error(), kw
    assert call(T=0) == 0 and call(P=0, fs=0) == 0 and call(T=0, tau=None) == 0, "empty: no launch"


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from cwfa_amd import ops
    from cwfa_amd.XLFMDataset import XLFMDatasetFull, extract_sparse
    s = torch.zeros(4, 3, 5)
    for call in (lambda: ops.temporal_select(s, [0]), lambda: ops.frame_dots(s, s[0]), lambda: ops.sparse_residual(s, s[:, 0, 0], s[0]),
                 lambda: extract_sparse(s)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError, match="float32 or float16"):
        ops.temporal_lds_frames(torch.float64)
    with pytest.raises(ValueError, match="contiguous"):
        extract_sparse(s[:, :, ::2])
    with pytest.raises(ValueError, match="scale"):
        extract_sparse(s, scale="mean")
    assert ops.temporal_lds_frames(torch.float16) == 2 * ops.temporal_lds_frames(torch.float32)
    assert ops.temporal_lds_frames(torch.float16, True) == ops.temporal_lds_frames(torch.float32, True)
    import inspect
    assert list(inspect.signature(XLFMDatasetFull.from_tensors).parameters) == ["raw_frames", "vols", "img_shape", "ds_id", "sparse"]
    assert inspect.signature(XLFMDatasetFull.from_tensors).parameters["sparse"].default is None
