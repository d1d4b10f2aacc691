"""GPU: the data preparation pass -- every mirror against the fixtures recorded from the reference
(tests/golden/g22_prep_*.npz) and the restatement of tests/prep_ref.py; the histogram kernel against torch.histogram on the CPU,
exactly; float64 device sums within 1e-8 relative (the project's bound for them, under 2^25 terms here).  Where a float64
result comes back as fp32 (the returned statistics, the per-voxel mean / std) the bound is the float64 restatement rounded once
to fp32: bit-equal for the means, one fp32 ulp (2^-23 = 1.2e-7 relative) for a std, whose square root is rounded too."""
import types

import numpy as np
import pytest
import torch

import prep_ref as R
from test_prep_cpu import CONFIGS, VOLUME_CALLS, assert_bits, golden, hist_corner_inputs

pytestmark = pytest.mark.gpu
ULP32 = 2.0 ** -23


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def corner_inputs():
    return hist_corner_inputs()


def test_volumes_match_the_reference():
    from cwfa_amd import utils as U
    z = golden("volumes")
    for vn in ("a", "b"):
        v, size = dev(z[f"vol_{vn}"]), [int(s) for s in z[f"size_{vn}"]]
        assert_bits(host(U.crop_volume_center(v, [1, size[2], size[0], size[1]])), z[f"crop_{vn}"], "crop")
        for cn, (ths, norm) in VOLUME_CALLS.items():
            out = U.load_process_volume(v, size, volume_ths=ths, norm=norm)
            assert out.dtype == torch.float16
            assert_bits(host(out), z[f"{vn}/{cn}"], f"{vn}/{cn}")
            with torch.autocast("cuda"):
                assert torch.equal(U.load_process_volume(v, size, volume_ths=ths, norm=norm), out)
        assert_bits(host(v), z[f"vol_{vn}"], "the input is left alone")
    v3 = dev(z["vol3"])
    assert_bits(host(U.load_process_volume(v3, [7, 8, 6], volume_ths=[24.0, 1000.0], norm=None, channel_order="xyz")), z["vol3/xyz"], "xyz")
    assert_bits(host(U.load_process_volume(v3, [8, 5, 6], volume_ths=[24.0, 1000.0], norm=None, channel_order="yxz")), z["vol3/yxz"], "yxz")


def test_frames_match_the_reference():
    from cwfa_amd import XLFMDataset as X
    z = golden("frames")
    raw = dev(z["raw"])
    for S in (40, 44):
        assert_bits(host(X.prepare_frames(raw, [S, S])), z[f"views_{S}"], f"views {S}")
    assert_bits(host(X.XLFMDatasetFull.from_tensors(raw, None, [40, 40]).stacked_views), z["views_40"], "from_tensors")


def test_quantile_matches_the_reference():
    from cwfa_amd import ops, utils as U
    z = golden("quantile")
    x = dev(z["x"])
    counts, edges = ops.histogram(x, 10000)
    assert np.array_equal(host(counts), z["counts"])
    assert_bits(edges.numpy(), z["edges"], "edges")
    for q in z["quants"]:
        got = U.fast_quantile(x, float(q))
        assert got.dtype == torch.float32 and got.dim() == 0 and not got.is_cuda
        assert_bits(got.numpy(), z[f"q{q}/value"], f"quantile {q}")
        with torch.autocast("cuda"):
            assert torch.equal(U.fast_quantile(x, float(q)), got)


def test_pipeline_matches_the_reference():
    from cwfa_amd import utils as U
    z, v = golden("pipeline"), golden("volumes")
    for cn, kw in CONFIGS.items():
        for n in ("a", "b"):
            ds = types.SimpleNamespace(vols=dev(v[f"vol_{n}"]), stacked_views=dev(z[f"views_{n}"]))
            assert U.prepare_XLFM_data(ds, [int(s) for s in v[f"size_{n}"]], **kw) is ds
            cast = types.SimpleNamespace(vols=dev(v[f"vol_{n}"]), stacked_views=dev(z[f"views_{n}"]))
            with torch.autocast("cuda"):                                         # fp16 volumes are data here, not autocast products
                U.prepare_XLFM_data(cast, [int(s) for s in v[f"size_{n}"]], **kw)
            assert cast.vols.dtype == torch.float32 and torch.equal(cast.vols, ds.vols) and torch.equal(cast.stacked_views, ds.stacked_views)
            assert ds.vols.dtype == torch.float32
            assert_bits(host(ds.vols), z[f"{cn}/{n}/vols"], f"{cn}/{n} volumes")
            assert_bits(host(ds.stacked_views), z[f"{cn}/{n}/views"], f"{cn}/{n} views")


def concat_of(z, prefix=""):
    from cwfa_amd import XLFMDataset as X
    sets = [X.XLFMDatasetFull(dev(z[f"{prefix}views_{k}"]), dev(z[f"{prefix}vols_{k}"])) for k in (0, 1)]
    return X.ConcatDataset(*sets), sets


def test_concat_dataset_matches_the_reference():
    from cwfa_amd import XLFMDataset as X
    z = golden("concat")
    both, sets = concat_of(z)
    vols, views = [z["vols_0"], z["vols_1"]], [z["views_0"], z["views_1"]]
    assert len(both) == int(z["len"])
    item = both[len(sets[0])]
    assert torch.equal(item[0], sets[1].stacked_views[[0]]) and torch.equal(item[1], sets[1].vols[0])
    stats = both.get_statistics()
    assert len(stats) == 6 and all(s.dtype == torch.float32 and s.dim() == 0 for s in stats)
    mi, si, _ = R.mean_std(views)
    mv, sv, _ = R.mean_std(vols)
    want = np.array([mi, si, mi, si, mv, sv])
    from cwfa_amd import ops
    got64 = ops.mean_std([t.stacked_views for t in sets])[:2] + ops.mean_std([t.vols for t in sets])[:2]
    print("statistics, relative to float64:", [f"{abs(a - b) / abs(b):.2e}" for a, b in zip(got64, (mi, si, mv, sv))])
    np.testing.assert_allclose(got64, [mi, si, mv, sv], rtol=1e-8)
    # the float64 statistic itself is within 1e-8; the returned value is that rounded to fp32 once
    np.testing.assert_array_equal(np.array([float(s) for s in stats], np.float32), want.astype(np.float32))
    np.testing.assert_allclose([float(s) for s in stats], z["stats"], rtol=1e-4)
    one = X.ConcatDataset(sets[0]).get_statistics()
    np.testing.assert_allclose([float(s) for s in one], z["stats_one"], rtol=1e-4)
    single = sets[0].get_statistics()
    np.testing.assert_array_equal([float(s) for s in single], [float(one[k]) for k in (0, 1, 4, 5)])
    m, s = both.mean(0), both.std(0)
    rm, rs = R.stack_mean_std(np.concatenate(vols))
    assert tuple(m.shape) == z["mean0"].shape
    np.testing.assert_array_equal(host(m)[0], rm.astype(np.float32))             # fp32 outputs of float64 sums: rounded once
    print("per-voxel std, relative to float64:", float(np.nanmax(np.abs(host(s)[0] - rs) / np.where(rs > 0, rs, 1))))
    np.testing.assert_allclose(host(s)[0], rs, rtol=ULP32, atol=0)
    pair = both.mean_std(0)
    assert torch.equal(pair[0], m) and torch.equal(pair[1], s)
    with torch.autocast("cuda"):
        assert torch.equal(both.mean(0), m) and torch.equal(both.std(0), s)
        assert all(torch.equal(a, b) for a, b in zip(both.get_statistics(), stats))
    np.testing.assert_allclose(host(m), z["mean0"], rtol=1e-4, atol=1e-30)
    np.testing.assert_allclose(host(s), z["std0"], rtol=1e-4, atol=1e-30)
    assert_bits(np.array([float(v) for v in both.get_max()], np.float32), z["max"], "get_max")
    assert both.get_max() is both.max_values                                     # cached, as the reference caches it
    assert_bits(np.array([float(v) for v in sets[0].get_max()], np.float32),
                np.array([views[0].max(), views[0].max(), vols[0].max()], np.float32), "get_max of one dataset")
    cast, cast_sets = concat_of(z)
    with torch.autocast("cuda"):
        assert all(torch.equal(a, b) for a, b in zip(cast.get_max(), both.get_max()))
        cast.normalize_datasets()
        cast.standarize_datasets([torch.tensor(t) for t in z["norm/stats"]])
    both.normalize_datasets()
    for k in (0, 1):
        assert_bits(host(sets[k].vols), z[f"norm/vols_{k}"], "normalised volumes")
        assert_bits(host(sets[k].stacked_views), z[f"norm/views_{k}"], "normalised views")
    np.testing.assert_allclose([float(t) for t in both.get_statistics()], z["norm/stats"], rtol=1e-4)
    both.standarize_datasets([torch.tensor(t) for t in z["norm/stats"]])         # the reference's own statistics: bit-equal maps
    for k in (0, 1):
        assert_bits(host(sets[k].vols), z[f"stand/vols_{k}"], "standardised volumes")
        assert_bits(host(sets[k].stacked_views), z[f"stand/views_{k}"], "standardised views")
        assert torch.equal(cast_sets[k].vols, sets[k].vols) and torch.equal(cast_sets[k].stacked_views, sets[k].stacked_views)


def test_stack_mean_std_edge_cases():
    from cwfa_amd import ops
    g = torch.Generator().manual_seed(3)
    for shape in ((1, 3, 5, 7), (5, 3, 5, 7), (4, 2, 8, 8), (3, 1, 1, 4099)):       # N = 1, scalar and 16-byte paths, several blocks
        x = torch.randn(shape, generator=g) * 0.01 + 1000
        m, s = ops.stack_mean_std(x.cuda())
        rm, rs = R.stack_mean_std(x.numpy())
        np.testing.assert_array_equal(host(m), rm.astype(np.float32))
        if shape[0] == 1:
            assert np.isnan(host(s)).all()
        else:
            np.testing.assert_allclose(host(s), rs, rtol=ULP32)                    # survives the mean of 1000: centred sums


@pytest.mark.parametrize("bins", [1, 7, 10000])
def test_histogram_is_torch_histogram(bins, corner_inputs):
    from cwfa_amd import ops
    for name, x in corner_inputs.items():
        want, want_edges = torch.histogram(x, bins=bins)
        counts, edges = ops.histogram(x.cuda(), bins)
        assert counts.dtype == torch.int64 and counts.is_cuda
        assert_bits(edges.numpy(), want_edges.numpy(), f"{name}: edges")
        got = host(counts)
        assert int(got.sum()) == x.numel()
        assert np.array_equal(got, want.numpy().astype(np.int64)), f"{name}: {int((got != want.numpy()).sum())} of {bins} bins differ"
    x = corner_inputs["n4099"].cuda()[1:]                                          # a base that is not 16-byte aligned
    assert np.array_equal(host(ops.histogram(x, bins)[0]), torch.histogram(x.cpu(), bins=bins)[0].numpy().astype(np.int64))


def test_histogram_accumulates_chunks(corner_inputs):
    from cwfa_amd import ops
    x = corner_inputs["f16grid"]
    rng = (x.min(), x.max())
    whole, _ = ops.histogram(x.cuda(), 10000)
    parts, _ = ops.histogram(x[:100_003].cuda(), 10000, range=rng)
    again, _ = ops.histogram(x[100_003:].cuda(), 10000, range=rng, counts=parts)
    assert again is parts and torch.equal(parts, whole)
    with pytest.raises(ValueError):
        ops.histogram(torch.tensor([1.0, float("inf")]).cuda(), 7)
    with pytest.raises(ValueError):
        ops.moments(torch.zeros(4).cuda(), float("nan"))


def test_chunked_statistics_agree():
    from cwfa_amd import XLFMDataset as X
    z = golden("concat")
    both, sets = concat_of(z)
    whole = X.ConcatDataset(X.XLFMDatasetFull(torch.cat([s.stacked_views for s in sets]), torch.cat([s.vols for s in sets])))
    from cwfa_amd import ops
    a, b = ops.mean_std([s.vols for s in sets]), ops.mean_std([torch.cat([s.vols for s in sets])])
    assert a[2] == b[2] == sum(s.vols.numel() for s in sets)
    np.testing.assert_allclose(a[:2], b[:2], rtol=1e-8)
    np.testing.assert_allclose([float(t) for t in both.get_statistics()], [float(t) for t in whole.get_statistics()], rtol=1e-8)


def test_moments_survive_a_large_mean():
    """The two-pass (c = 0, then c = mean) statistics within 1e-8 of the float64 restatement on 1000 + randn.  The std formed from
    the c = 0 sums alone is printed beside it, not asserted: sum x^2 is about 1e12 against n * var of about 1e6, so its relative
    error is about 1e6 times that of a float64 sum, which stays inside 1e-8 (1.4e-10 with numpy's float64 sums): at this ratio the
    second pass is a safety margin.  test_centring_is_needed_for_a_narrow_spread holds the case where it is required."""
    from cwfa_amd import ops
    x = 1000 + torch.randn(1 << 20, generator=torch.Generator().manual_seed(11))
    rm, rs, n = R.mean_std([x.numpy()])
    m, s, cnt = ops.mean_std([x.cuda()])
    assert cnt == n
    print(f"moments: mean rel {abs(m - rm) / rm:.3e}, std rel {abs(s - rs) / rs:.3e}")
    np.testing.assert_allclose([m, s], [rm, rs], rtol=1e-8)
    raw = ops.moments(x.cuda()).tolist()
    np.testing.assert_allclose(raw[0], x.double().sum().item(), rtol=1e-12)
    assert raw[2] == n
    s0 = ((raw[1] - raw[0] * raw[0] / n) / (n - 1)) ** 0.5                          # the std from the uncentred (c = 0) sums
    print(f"moments: std from the uncentred sums, rel {abs(s0 - rs) / rs:.3e}")
    sparse = torch.stack([x[: 1 << 10], 2 * x[: 1 << 10]], dim=-1).reshape(4, 16, 16, 2).cuda()
    from cwfa_amd import XLFMDataset as X
    st = X.ConcatDataset(X.XLFMDatasetFull(sparse, x[:64].reshape(4, 1, 4, 4).cuda())).get_statistics()
    np.testing.assert_allclose([float(st[0]), float(st[2])], [x[: 1 << 10].double().mean().item(), 2 * x[: 1 << 10].double().mean().item()], rtol=ULP32)
    np.testing.assert_allclose(float(st[3]), 2 * float(st[1]), rtol=ULP32)


def test_centring_is_needed_for_a_narrow_spread():
    """1e4 + 0.01 * randn, 2^20 elements: sum x^2 is about n * 1e8 against n * var = n * 1e-4, so one float64 rounding of the
    uncentred sums (1.1e-16 relative) already moves the variance by about 1e-4 relative: the std formed from the c = 0 sums alone
    misses the 1e-8 bound, the centred second pass keeps it."""
    from cwfa_amd import ops
    x = 1e4 + 0.01 * torch.randn(1 << 20, generator=torch.Generator().manual_seed(12))
    rm, rs, n = R.mean_std([x.numpy()])
    m, s, cnt = ops.mean_std([x.cuda()])
    s1, s2, _ = ops.moments(x.cuda()).tolist()
    s0 = max((s2 - s1 * s1 / n) / (n - 1), 0.0) ** 0.5
    print(f"narrow spread: two-pass std rel {abs(s - rs) / rs:.3e}, from the uncentred sums rel {abs(s0 - rs) / rs:.3e}")
    assert cnt == n
    np.testing.assert_allclose([m, s], [rm, rs], rtol=1e-8)
    assert abs(s0 - rs) / rs > 1e-8


def test_full_size_level():
    from cwfa_amd import XLFMDataset as X, ops, utils as U
    g = torch.Generator().manual_seed(22)
    shape = (2, 96, 512, 512)
    v = torch.where(torch.rand(shape, generator=g) < 0.7, torch.zeros(()), torch.rand(shape, generator=g) * 900).half()
    ths = [24.0, 800.0]
    want = R.prep_volumes(v.numpy(), 512, 512, ths, None).astype(np.float32)
    runs = []
    for _ in range(2):
        ds = types.SimpleNamespace(vols=v.cuda(), stacked_views=torch.ones(2, 8, 8).cuda())
        U.prepare_XLFM_data(ds, [512, 512, 96], ths, [0.0, 1], [0.0, 1.0], None)
        counts, _ = ops.histogram(ds.vols, 10000)
        stats = X.ConcatDataset(X.XLFMDatasetFull(ds.stacked_views, ds.vols)).get_statistics()
        runs.append((ds.vols, counts, torch.stack(stats)))
    assert_bits(host(runs[0][0]), want, "prepared volume")
    ref_counts = torch.histogram(torch.from_numpy(want), bins=10000)[0]
    got = host(runs[0][1])
    # bin 0 (the background alone: the lowest value above it is 24) holds more than 2^24 elements, beyond the integers of the fp32
    # counts torch.histogram keeps on the CPU: it is checked against the exact count, every other bin against torch
    assert np.array_equal(got[1:], ref_counts.numpy().astype(np.int64)[1:])
    assert got[0] == int((want == 0).sum()) > 2 ** 24 and int(got.sum()) == want.size
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    mv, sv, _ = R.mean_std([want])
    np.testing.assert_allclose([float(runs[0][2][4]), float(runs[0][2][5])], [mv, sv], rtol=ULP32)
