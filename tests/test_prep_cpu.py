"""CPU: the data preparation pass without a device -- the float64 / numpy restatement (tests/prep_ref.py)
against the fixtures recorded from the reference, the restated bin rule against torch.histogram, and the host halves of the
mirrors (index maps, the quantile walk, argument checks, unsupported arguments)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import prep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cwfa_prep_volumes_f16", "cwfa_prep_frames_f32", "cwfa_histogram_f32", "cwfa_prep_apply_f32", "cwfa_moments_f64",
         "cwfa_stack_mean_std_f32"]
VOLUME_CALLS = {"none": ([], None), "two": ([24.0, 1000.0], None), "float": (0.05, None), "max": (0.1, "max")}
CONFIGS = {"two_q": dict(volume_ths=[24.0, 1000.0], volume_quantiles=[0.0, 0.9], img_ths=[0.3, 1.0], norm=None),
           "float_noq": dict(volume_ths=0.05, volume_quantiles=[0.0, 1], img_ths=[0.1, 1.0], norm=None),
           "max_q": dict(volume_ths=0.1, volume_quantiles=[0.0, 0.97], img_ths=[0.5, 1.0], norm="max")}


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"g22_prep_{name}.npz"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), f"{what}: {int((bits(got) != bits(want)).sum())} elements differ"


def hist_corner_inputs():
    """name -> float32 tensor: the inputs of the histogram tests (CPU restatement and device kernel alike)."""
    g = torch.Generator().manual_seed(0)
    out = {}
    for n in (1, 63, 64, 65, 4099, 3 * 7 * 129 * 130):
        out[f"n{n}"] = torch.rand(n, generator=g) * 5 - 2
    out["all_equal"] = torch.full((1000,), 3.25)
    z = torch.zeros(200_000)
    z[torch.randperm(200_000, generator=g)[:200]] = torch.rand(200, generator=g) * 100 + 1
    out["zeros999"] = z
    out["hi_or_lo"] = torch.where(torch.rand(50_001, generator=g) < 0.5, torch.tensor(-1.5), torch.tensor(7.0))
    out["f16grid"] = (torch.rand(300_000, generator=g) * 20000).half().float()
    out["uniform"] = torch.rand(2_000_000, generator=torch.Generator().manual_seed(0))
    return out


# ---------------------------------------------------------------------------------------------- restatement vs fixtures
def test_restated_volumes_match_the_reference():
    z = golden("volumes")
    for vn in ("a", "b"):
        size = z[f"size_{vn}"]
        (h0, h1), (w0, w1) = R.crop_range(z[f"vol_{vn}"].shape[2], size[0]), R.crop_range(z[f"vol_{vn}"].shape[3], size[1])
        assert_bits(z[f"vol_{vn}"][:, :, h0:h1, w0:w1], z[f"crop_{vn}"], "crop")
        for cn, (ths, norm) in VOLUME_CALLS.items():
            assert_bits(R.prep_volumes(z[f"vol_{vn}"], size[0], size[1], ths, norm), z[f"{vn}/{cn}"], f"{vn}/{cn}")
    assert int((z["a/two"] == 1000).sum()) >= 1 and float((z["a/two"] == 0).mean()) > 0.6
    assert z["raised_resize"] == 1


def test_restated_frames_match_the_reference():
    z = golden("frames")
    assert np.isnan(z["raw"]).sum() == 1 and np.isinf(z["raw"]).sum() == 2
    for S in (40, 44):
        assert_bits(R.prep_frames(z["raw"], S, S), z[f"views_{S}"], f"views {S}")
    assert tuple(z["padded_shape"]) == (45, 44)                    # the odd difference: one column more than half off each side


def test_restated_quantile_matches_the_reference():
    z = golden("quantile")
    counts, edges = R.histogram(z["x"], 10000)
    assert np.array_equal(counts, z["counts"])
    assert_bits(edges, z["edges"], "edges")
    crossed = []
    for q in z["quants"]:
        e, n_bin, c, above, below = R.quantile_walk(counts, edges, float(q))
        assert_bits(e, z[f"q{q}/value"], f"quantile {q}")
        assert int(c) == int(z[f"q{q}/crossed"])
        assert not c or (above >= 2 and below >= 2)
        crossed.append(c)
    assert any(crossed) and not all(crossed)
    assert R.quantile_walk(counts, edges, 0.99999)[0] == edges[9999] != edges[10000]


def test_restated_pipeline_matches_the_reference():
    z, v = golden("pipeline"), golden("volumes")
    for cn, kw in CONFIGS.items():
        for n in ("a", "b"):
            vols, views, upper, low = R.prepare(v[f"vol_{n}"], z[f"views_{n}"], v[f"size_{n}"], **kw)
            assert_bits(vols, z[f"{cn}/{n}/vols"], f"{cn}/{n} volumes")
            assert_bits(views, z[f"{cn}/{n}/views"], f"{cn}/{n} views")
            if upper is not None:
                assert vols.max() == upper


def test_restated_statistics_match_the_reference():
    z = golden("concat")
    vols, views = [z["vols_0"], z["vols_1"]], [z["views_0"], z["views_1"]]
    mi, si, _ = R.mean_std(views)
    mv, sv, n = R.mean_std(vols)
    assert n == vols[0].size * 2
    np.testing.assert_allclose([mi, si, mi, si, mv, sv], z["stats"], rtol=1e-4)
    np.testing.assert_allclose(R.mean_std(views[:1])[:2] * 2 + R.mean_std(vols[:1])[:2], z["stats_one"], rtol=1e-4)
    m, s = R.stack_mean_std(np.concatenate(vols))
    assert z["mean0"].shape == (1,) + m.shape
    np.testing.assert_allclose(m, z["mean0"][0], rtol=1e-4, atol=1e-30)
    np.testing.assert_allclose(s, z["std0"][0], rtol=1e-4, atol=1e-30)
    mx = [max(a.max() for a in views)] * 2 + [max(a.max() for a in vols)]
    assert_bits(np.array(mx, np.float32), z["max"], "max")
    for k in (0, 1):
        assert_bits(R.apply(vols[k], "div_mul", vols[k].max(), mx[2]), z[f"norm/vols_{k}"], "normalised volumes")
        assert_bits(R.apply(views[k], "div_mul", views[k].max(), mx[0]), z[f"norm/views_{k}"], "normalised views")
        st = z["norm/stats"]
        assert_bits(R.apply(z[f"norm/vols_{k}"], "sub_div", st[4], st[5]), z[f"stand/vols_{k}"], "standardised volumes")
        assert_bits(R.apply(z[f"norm/views_{k}"], "sub_div", st[0], st[1]), z[f"stand/views_{k}"], "standardised views")


# ---------------------------------------------------------------------------------------------- the bin rule
@pytest.mark.parametrize("bins", [1, 7, 10000])
def test_restated_bin_rule_is_torch_histogram(bins):
    plain_wrong = 0
    for name, x in hist_corner_inputs().items():
        want, want_edges = torch.histogram(x, bins=bins)
        counts, edges = R.histogram(x.numpy(), bins)
        assert_bits(edges, want_edges.numpy(), f"{name}: edges")
        assert np.array_equal(counts, want.numpy().astype(np.int64)), f"{name}: {int((counts != want.numpy()).sum())} bins differ"
        lo, hi = R.hist_range(x.min(), x.max())
        plain = np.bincount(R.hist_bins_plain(x.numpy(), lo, hi, bins), minlength=bins)
        plain_wrong += int((plain != counts).sum())
    assert bins != 10000 or plain_wrong > 0                         # the search among the edges is not decoration


# ---------------------------------------------------------------------------------------------- host halves of the mirrors
def test_index_maps():
    from cwfa_amd import XLFMDataset as X, utils as U
    for full in range(1, 12):
        for crop in range(0, full + 1):
            assert U.crop_offsets(full, crop) == R.crop_range(full, crop)
            assert U.crop_offsets(full, crop)[1] - U.crop_offsets(full, crop)[0] == crop
    with pytest.raises(ValueError):
        U.crop_offsets(4, 5)
    z = golden("frames")
    raw = torch.from_numpy(z["raw"])
    padded = X.pad_img_to_min(raw[0])
    assert tuple(padded.shape) == tuple(z["padded_shape"])
    for S in (40, 44):
        assert X.frame_offsets(45, 52, [S, S]) == R.frame_offsets(45, 52, S, S)
        assert_bits(X.center_crop(padded[None, None], [S, S])[0, 0].numpy(), z[f"center_crop_{S}"], "center_crop")
        oy, ox = X.frame_offsets(45, 52, [S, S])
        assert_bits(raw[0, oy:oy + S, ox:ox + S].numpy(), z[f"center_crop_{S}"], "offsets")
    assert X.frame_offsets(52, 45, [44, 40]) == (4, 2) and X.frame_offsets(6, 6, [6, 6]) == (0, 0)
    with pytest.raises(ValueError):
        X.frame_offsets(45, 52, [45, 45])                           # 44 columns are left
    v = torch.zeros(1, 2, 7, 8)
    assert tuple(U.crop_volume_center(v, [1, 2, 4, 5]).shape) == (1, 2, 4, 5)


def test_quantile_walk_of_the_mirror():
    from cwfa_amd import utils as U
    z = golden("quantile")
    h, edges = torch.from_numpy(z["counts"]).float(), torch.from_numpy(z["edges"])
    for q in z["quants"]:
        got = U.quantile_walk(h, edges, float(q))
        assert got.dtype == torch.float32 and got.dim() == 0
        assert_bits(got.numpy(), z[f"q{q}/value"], f"quantile {q}")
    g = torch.Generator().manual_seed(5)
    for _ in range(20):                                              # against the literal walk, counts beyond fp32's integers included
        c = torch.randint(0, 40_000_000, (50,), generator=g)
        e = torch.linspace(0, 1, 51)
        q = float(torch.rand((), generator=g))
        assert float(U.quantile_walk(c.float(), e, q)) == float(R.quantile_walk(c.numpy(), e.numpy(), q)[0])
    assert float(U.quantile_walk(torch.zeros(10), torch.linspace(0, 1, 11), 0.5)) == float(torch.linspace(0, 1, 11)[1])
    with pytest.raises(ValueError):
        U.quantile_walk(torch.ones(1), torch.tensor([0.0, 1.0]), 0.5)


def test_unsupported_arguments_and_cpu_tensors():
    from cwfa_amd import XLFMDataset as X, ops, utils as U
    v = torch.zeros(1, 2, 8, 8, dtype=torch.float16)
    with pytest.raises(NotImplementedError):
        U.load_process_volume("volume.h5", [8, 8, 2])
    with pytest.raises(NotImplementedError):
        U.load_process_volume(v, [8, 8, 2], volume_ths=0.1, norm="std")
    with pytest.raises(NotImplementedError):
        U.load_process_volume(v, [8, 8, 2], volume_ths=0.1, resize=True)
    with pytest.raises(TypeError):
        U.load_process_volume(v.float(), [8, 8, 2], volume_ths=0.1)
    with pytest.raises(ValueError):
        U.load_process_volume(v, [9, 8, 2], volume_ths=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.load_process_volume(v, [8, 8, 2], volume_ths=0.1)
    for call in (lambda: U.fast_quantile(torch.zeros(8)), lambda: X.prepare_frames(torch.zeros(1, 8, 8), [4, 4]),
                 lambda: ops.histogram(torch.zeros(8)), lambda: ops.moments(torch.zeros(8)), lambda: ops.stack_mean_std(torch.zeros(2, 8)),
                 lambda: ops.prep_apply(torch.zeros(8), "sub_div", 0.0, 1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(NotImplementedError):
        X.ConcatDataset(X.XLFMDatasetFull(torch.zeros(1, 4, 4), torch.zeros(1, 2, 4, 4))).mean(1)
    with pytest.raises(ValueError):
        ops.histogram_range(0.0, float("inf"))
    lo, hi = ops.histogram_range(3.25, 3.25)
    assert (float(lo), float(hi)) == (2.75, 3.75)
    assert not hasattr(X.ConcatDataset, "add_random_shot_noise_to_dataset")


def test_entry_points_validate_without_a_device():
    from cwfa_amd import _lib, build
    build.build_all()
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.cwfa_prep_volumes_f16(None, p, None, 1, 1, 4, 4, 4, 4, 0, 0, 0, 0.0, 0.0, 0, None) == -1
    assert L.cwfa_prep_volumes_f16(p, p, None, 1, 1, 4, 4, 4, 4, 0, 0, 3, 0.0, 0.0, 0, None) == -1          # maxnorm needs maxbuf
    assert L.cwfa_prep_volumes_f16(p, p, p, 1, 1, 4, 4, 4, 4, 1, 0, 0, 0.0, 0.0, 0, None) == -2             # crop leaves the plane
    assert b"crop" in L.cwfa_last_error()
    assert L.cwfa_prep_volumes_f16(p, p, p, 1, 1, 4, 4, 4, 4, 0, 0, 9, 0.0, 0.0, 0, None) == -1
    assert L.cwfa_prep_volumes_f16(p, p, p, 0, 1, 4, 4, 4, 4, 0, 0, 0, 0.0, 0.0, 0, None) == 0
    assert L.cwfa_prep_frames_f32(None, p, 1, 4, 4, 4, 4, 0, 0, None) == -1
    assert L.cwfa_prep_frames_f32(p, p, 1, -4, 4, 4, 4, 0, 0, None) == -2
    assert L.cwfa_prep_frames_f32(p, p, 0, 4, 4, 4, 4, 0, 0, None) == 0
    assert L.cwfa_histogram_f32(p, 8, 0.0, 1.0, p, 0, p, 0, None) == -1
    assert L.cwfa_histogram_f32(p, 8, 0.0, 1.0, p, _lib.PREP_MAX_BINS + 1, p, 0, None) == -1
    assert L.cwfa_histogram_f32(p, 8, 1.0, 1.0, p, 8, p, 0, None) == -1 and b"range" in L.cwfa_last_error()
    assert L.cwfa_histogram_f32(p, 8, 0.0, float("inf"), p, 8, p, 0, None) == -1
    assert L.cwfa_histogram_f32(p, 8, 0.0, 1.0, None, 8, p, 0, None) == -1
    assert L.cwfa_prep_apply_f32(p, 8, 3, 0.0, 0.0, 0, None) == -1
    assert L.cwfa_prep_apply_f32(p, 8, 0, 0.0, 0.0, 4, None) == -1
    assert L.cwfa_prep_apply_f32(None, 0, 0, 0.0, 0.0, 0, None) == 0
    assert L.cwfa_moments_f64(p, 8, float("nan"), p, p, 0, None) == -1
    assert L.cwfa_moments_f64(p, 8, 0.0, None, p, 0, None) == -1
    assert L.cwfa_stack_mean_std_f32(p, p, p, 0, 8, 8, None) == -2
    assert L.cwfa_stack_mean_std_f32(p, p, p, 2, 8, 4, None) == -1
    assert L.cwfa_stack_mean_std_f32(p, p, p, 2, 0, 0, None) == 0


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "cwfa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from cwfa_amd import _lib
    for n in NAMES:
        assert re.search(rf"\bint {n}\s*\(", src), n
        assert n in _lib.SIGNATURES
    assert open(os.path.join(ROOT, "cwfa_amd", "build.py")).read().count('"prep_ops.hip"') == 1
