"""CPU: the evaluation pass without a GPU -- the float64 restatement (tests/eval_ref.py) against the reference's recorded results
(tests/golden/g21_eval_*.npz, written by tools/make_eval_golden.py), the host parts of the mirrors, and the argument validation of
the six new entry points.  Bounds: bit-exact for raw volumes, composites and index ranges; 1e-4 (conftest.assert_close, the
project's bound) against the reference's fp32 sums."""
import ctypes

import numpy as np
import pytest
from conftest import assert_close, load_golden

import eval_ref as R

CORR = ["g21_eval_corr_bright_fw10", "g21_eval_corr_bright_fw0", "g21_eval_corr_dim_fw10", "g21_eval_corr_dim_fw0"]
PROJ = {"default": {}, "depths_in_ch": {}, "normalize": dict(normalize=True), "ths": dict(ths=(0.1, 0.9)),
        "normalize_ths": dict(normalize=True, ths=(0.1, 0.9)), "bars": dict(bars=True), "scale3_border3": dict(depth_scale=3, border=3),
        "all": dict(normalize=True, ths=(0.2, 0.7), bars=True, depth_scale=4, border=1)}


def metric_cases(fx):
    for name in fx["cases"]:
        name = str(name)
        step, norm, ths = int(name[1]), name[4] == "1", (0.05 if name[-1] == "1" else 0.0)
        yield name, step, norm, ths


def stacks_of(fx):
    T, D, H, W = (int(v) for v in fx["shape"])
    bg = float(fx["bg"])
    sg = R.make_stack(int(fx["seeds"][0]), T, (D, H, W), fx["boxes"], fx["act_gt"], bg, bg / 4)
    sp = R.make_stack(int(fx["seeds"][1]), T, (D, H, W), fx["boxes"], fx["act_pred"], bg, bg / 4)
    assert sg.astype(np.float64).sum() == fx["checksum"][0] and sp.astype(np.float64).sum() == fx["checksum"][1], \
        "the rebuilt stacks are not the ones the fixture was recorded on"
    return sg, sp


def assert_frame(values, want):
    """The data frame of corr_coeff_3D against the recorded one: the traces (columns 6 ..) on their own to the 1e-4 of
    conftest.assert_close (they lie in [0, 1]; the coordinate columns would dominate a norm over the whole frame), patch number,
    coordinates and is_gt exactly, the coefficient column to 1e-4 as well."""
    assert values.shape == want.shape and np.array_equal(np.isnan(values), np.isnan(want))
    assert np.array_equal(values[:, :4], want[:, :4]) and np.array_equal(values[:, 5], want[:, 5]), "patch_n / coordinates / is_gt"
    assert_close(np.nan_to_num(values[:, 4]), np.nan_to_num(want[:, 4]), what="corr_coeff column")
    assert_close(np.nan_to_num(values[:, 6:]), np.nan_to_num(want[:, 6:]), what="traces")


def test_restatement_metrics_match_reference():
    fx = load_golden("g21_eval_metrics")
    for name, step, norm, ths in metric_cases(fx):
        p, m, graw, praw = R.step_performance(fx["gt"], fx["pred"], step, fx["mean"], fx["std"], norm, ths)
        if int(fx[name + "/raised"]):                      # ths == 0: the reference raises; PSNR does not depend on ths
            ref_p = float(fx[name[:-1] + "1/psnr"])
            assert abs(p - ref_p) <= 1e-4 * abs(ref_p)
            assert m == pytest.approx(np.abs(graw.astype(np.float64) - praw).mean() * 100, rel=1e-12)
            continue
        assert abs(p - float(fx[name + "/psnr"])) <= 1e-4 * abs(float(fx[name + "/psnr"])), name
        assert abs(m - float(fx[name + "/mape"])) <= 1e-4 * abs(float(fx[name + "/mape"])), name
        if name + "/gt_raw" in fx:
            assert np.array_equal(graw, fx[name + "/gt_raw"]) and np.array_equal(praw, fx[name + "/pred_raw"]), name
    ps, ms = R.step_performance(fx["same"], fx["same"], 1, fx["mean"], fx["std"])[:2]          # mse == 0, a non-zero image: 100
    assert ps == 100.0 == float(fx["same/psnr"]) and abs(ms - float(fx["same/mape"])) <= 1e-4 * float(fx["same/mape"])
    zero = np.zeros_like(fx["same"])
    assert R.step_performance(zero, zero, 1, 0.0, fx["std"])[:2] == (0.0, 0.0) == (float(fx["zero/psnr"]), float(fx["zero/mape"]))


@pytest.mark.parametrize("name", sorted(PROJ))
def test_restatement_projections_bit_exact(name):
    fx = load_golden("g21_eval_projections")
    out = R.projections(fx["vol"], **PROJ[name])
    assert out.shape == fx["out/" + name].shape and np.array_equal(out, fx["out/" + name])
    assert int(fx["nonsquare_raised"]) == 1 and int(fx["scaled_plane_raised"]) == 1


@pytest.mark.parametrize("name", CORR)
def test_restatement_corr_coeff_matches_reference(name):
    fx = load_golden(name)
    sg, sp = stacks_of(fx)
    coords = [tuple(int(v) for v in c) for c in fx["coords"]]
    ccs, values, index = R.corr_coeff(sg, sp, coords, int(fx["r12"]), int(fx["r3"]), filter_width=int(fx["filter_width"]))
    assert len(ccs) == len(fx["ccs"]) and list(index) == list(fx["df_index"])
    assert np.array_equal(np.isnan(ccs), np.isnan(fx["ccs"])) and np.array_equal(np.isnan(values), np.isnan(fx["df_values"]))
    assert_close(np.nan_to_num(ccs), np.nan_to_num(fx["ccs"]), what="correlation coefficients")
    assert_frame(values, fx["df_values"])


@pytest.mark.parametrize("name", CORR[::2])
def test_roi_boxes_match_recorded_ranges(name):
    from cwfa_amd.CWFA import roi_boxes
    fx = load_golden(name)
    got = roi_boxes([tuple(c) for c in fx["coords"]], tuple(fx["shape"]), int(fx["r12"]), int(fx["r3"]))
    assert got.dtype == np.int32 and np.array_equal(got, fx["boxes"]) and np.array_equal(R.roi_boxes(fx["coords"], fx["shape"], 5, 3), got)
    assert (got[-1, 1] - got[-1, 0]) == 0                     # the ROI outside in depth
    assert got[:, 0].min() == 0 and got[:, 1].max() == fx["shape"][1] and got[:, 2].min() == 0 and got[:, 5].max() == fx["shape"][3]


@pytest.mark.parametrize("name", CORR)
def test_host_glue_on_recorded_traces(name):
    """norm_data, the range gate, the halving loop and the data frame of the mirror, fed with float64 traces computed on the CPU."""
    from cwfa_amd.CWFA import correlate_traces
    from cwfa_amd.utils import filter_data, norm_data
    fx = load_golden(name)
    sg, sp = stacks_of(fx)
    coords = [tuple(int(v) for v in c) for c in fx["coords"]]
    mg, mp = sg.max(), sp.max()
    median = np.float32(R.select_positive(sg)[0]) / mg
    T, D = int(fx["shape"][0]), int(fx["shape"][1])
    ccs, df = correlate_traces(coords, fx["boxes"], R.roi_means(sg, fx["boxes"]) / np.float64(mg), R.roi_means(sp, fx["boxes"]) / np.float64(mp),
                               median, D // 2 + (-25 // 2), T, 50, int(fx["filter_width"]))
    assert list(df.columns) == [str(c) for c in fx["df_columns"]] and list(df.index) == list(fx["df_index"])
    assert len(ccs) == len(fx["ccs"]) == (len(coords) if int(fx["n_sweeps"]) == 1 else len(coords) + 2)
    assert_close(np.nan_to_num(np.array(ccs, dtype=np.float64)), np.nan_to_num(fx["ccs"]), what="correlation coefficients")
    assert_frame(df.to_numpy(dtype=np.float64), fx["df_values"])
    x = np.arange(12.0)
    assert np.allclose(filter_data(x, 4), np.convolve(x, np.ones(4) / 4, mode="same"))
    d, rng = norm_data(x + 1, 0)
    assert rng == 11 and np.allclose(d, x / 12)               # divided by the maximum, not the range
    assert norm_data(np.zeros(5), 0)[0].tolist() == [0.0] * 5


def test_mirrors_reject_cpu_tensors_and_callables():
    import torch
    from cwfa_amd import CWFA, utils
    v = torch.zeros(1, 4, 6, 6)
    for call in (lambda: utils.psnr(v, v), lambda: utils.volume_2_projections(v, depths_in_ch=True),
                 lambda: CWFA.compute_INN_step_performance(v, v, 0, 0.0, 1.0), lambda: CWFA.evaluate_step(v, v, 0, 0.0, 1.0),
                 lambda: CWFA.corr_coeff_3D(v, v, [(1, 1, 1)], 2, 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(NotImplementedError):
        utils.volume_2_projections(v, proj_type=torch.sum, depths_in_ch=True)
    with pytest.raises(NotImplementedError):
        CWFA.corr_coeff_3D(v, v, [(1, 1, 1)], 2, 1, output_path="x.pdf")
    import cwfa_amd
    import sys
    cwfa_amd.install()
    assert sys.modules.get("utils") is not utils


def test_argument_validation_without_gpu():
    from cwfa_amd import _lib, build
    build.build_all()
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # null pointers
    assert L.cwfa_volume_extrema_f32(None, None, p, p, 1, 8, 8, 8, None, None) == -1 and b"null" in L.cwfa_last_error()
    assert L.cwfa_volume_metrics_f32(p, None, p, p, 1, 8, 8, 8, None, 0.0, 0.0, 0.0, None) == -1
    assert L.cwfa_volume_metrics_f32(p, p, p, None, 1, 8, 8, 8, None, 0.0, 0.0, 0.0, None) == -1
    assert L.cwfa_mip3_f32(p, None, p, p, None, p, 1, 2, 2, 2, 8, 0, 0, None, None, None) == -1
    assert L.cwfa_mip3_f32(p, None, p, p, p, p, 1, 2, 2, 2, 8, 0, 1, None, None, None) == -1 and b"both tensors" in L.cwfa_last_error()
    assert L.cwfa_mip3_f32(p, p, p, p, p, p, 1, 2, 2, 2, 8, 8, 1, None, ctypes.byref(_lib.EvalPost()), None) == -1
    assert L.cwfa_projection_compose_f32(p, p, p, None, p, 1, 2, 4, 4, 2, 2, 0, None) == -1
    assert L.cwfa_roi_means_f32(None, p, p, 1, 2, 2, 2, 1, 8, None) == -1
    assert L.cwfa_select_positive_f32(p, 1, 8, 8, 0, None, p, p, None) == -1
    # negative sizes, strides smaller than a sample
    assert L.cwfa_volume_extrema_f32(p, None, p, p, -1, 8, 8, 8, None, None) == -2
    assert L.cwfa_volume_extrema_f32(p, None, p, p, 2, 8, 4, 0, None, None) == -1 and b"stride" in L.cwfa_last_error()
    assert L.cwfa_volume_metrics_f32(p, p, p, p, 1, -8, 8, 8, None, 0.0, 0.0, 0.0, None) == -2
    assert L.cwfa_mip3_f32(p, None, p, p, p, p, 1, -2, 2, 2, 8, 0, 0, None, None, None) == -2
    assert L.cwfa_projection_compose_f32(p, p, p, p, p, 1, 2, 4, 4, 0, 2, 0, None) == -1          # depth factor < 1
    assert L.cwfa_projection_compose_f32(p, p, p, p, p, 1, 2, 4, 6, 2, 2, 0, None) == -2 and b"square" in L.cwfa_last_error()
    assert L.cwfa_roi_means_f32(p, p, p, -1, 2, 2, 2, 1, 8, None) == -2
    assert L.cwfa_select_positive_f32(p, 1, -8, 8, 0, p, p, p, None) == -2
    # a box outside the tensor, an inverted box
    for bad in ([0, 3, 0, 2, 0, 2], [0, 2, 0, 2, -1, 2], [1, 0, 0, 2, 0, 2]):
        box = (ctypes.c_int32 * 6)(*bad)
        assert L.cwfa_roi_means_f32(p, box, p, 1, 2, 2, 2, 1, 8, None) == -1 and b"not inside" in L.cwfa_last_error()
    # k at or beyond the number of elements, k below -1
    assert L.cwfa_select_positive_f32(p, 1, 8, 8, 8, p, p, p, None) == -1 and b"not below" in L.cwfa_last_error()
    assert L.cwfa_select_positive_f32(p, 1, 8, 8, -2, p, p, p, None) == -1
    # workspace sizing and the measurement-only option
    assert L.cwfa_eval_splits(1, 96 * 512 * 512) == 2048 and L.cwfa_eval_splits(300, 96 * 512 * 512) == 7 and L.cwfa_eval_splits(2, 100) == 1
    assert L.cwfa_eval_splits(0, 8) == 0 and L.cwfa_eval_splits(1, -1) == -1
    assert L.cwfa_set_option(b"mip3_ablate", 8) == -1 and L.cwfa_set_option(b"mip3_ablate", 0) == 0
    # empty problems are accepted and launch nothing
    assert L.cwfa_volume_extrema_f32(p, None, p, p, 0, 8, 8, 8, None, None) == 0
    assert L.cwfa_volume_metrics_f32(p, p, p, p, 1, 0, 0, 0, None, 0.0, 0.0, 0.0, None) == 0
    assert L.cwfa_mip3_f32(p, None, p, p, p, p, 1, 0, 2, 2, 0, 0, 0, None, None, None) == 0
    assert L.cwfa_projection_compose_f32(p, p, p, p, p, 0, 2, 4, 4, 2, 2, 0, None) == 0
    assert L.cwfa_roi_means_f32(p, None, p, 4, 2, 2, 2, 0, 8, None) == 0
    assert L.cwfa_select_positive_f32(p, 0, 8, 8, 0, p, p, p, None) == 0
