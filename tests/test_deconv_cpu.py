"""CPU: the Richardson-Lucy deconvolution without a GPU -- the restatement (tests/deconv_ref.py) against the reference's recorded
results (tests/golden/g25_deconv_*.npz, written by tools/make_deconv_golden.py): bit-equal in float32, within the recorded
dev_ref in float64; the argument validation of the six new entry points through the built library; and the errors the mirrors of
cwfa_amd.utils decide before any launch."""
import ctypes

import numpy as np
import pytest
import torch
from conftest import load_golden

import deconv_ref as R

RL = {"i": (1,), "ii": (1,), "iii": (1, 2), "iv": (1,)}
SPLIT = ["odd_h", "odd_h2", "even"]


def rl(name):
    return load_golden(f"g25_deconv_rl_{name}")


def rel(a, b):
    wide = np.complex128 if np.iscomplexobj(a) else np.float64
    return float(np.abs(np.asarray(a, dtype=wide) - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def L():
    from cwfa_amd import _lib, build
    build.build_all()
    return _lib.lib()


@pytest.fixture(scope="module")
def ptr():
    buf = ctypes.create_string_buffer(4096)
    return ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("name", list(RL))
def test_restatement_reproduces_the_reference_deconvolution(name):
    z = rl(name)
    OTF, img = torch.from_numpy(z["OTF"]), torch.from_numpy(z["img"])
    obj, roi, nIt = [int(v) for v in z["ObjSize"]], [int(v) for v in z["ROIsize"]], int(z["nIt"])
    assert (z["img"][:, :, :3] == 0).all() and (OTF.ndim == 5) == (name == "iv")
    for ns in RL[name]:
        k = f"n{ns}/"
        vol, est, pad, pad_img, done = R.xlfm_deconv(OTF, img, nIt, obj, roi, ns, int(z["mult"]), torch.float32)
        assert done == nIt and np.array_equal(vol.numpy(), z[k + "vol"]) and np.array_equal(est.numpy(), z[k + "est"]), "fp32 bits"
        assert pad == list(z[k + "padSize"]) and pad_img == list(z[k + "padSizeImg"])
        v64, e64 = R.xlfm_deconv(OTF, img, nIt, obj, roi, ns, int(z["mult"]), torch.float64)[:2]
        assert rel(z[k + "vol"], v64.numpy()) <= float(z[k + "dev_vol"]) * (1 + 1e-6) < 2e-6
        assert rel(z[k + "est"], e64.numpy()) <= float(z[k + "dev_est"]) * (1 + 1e-6) < 2e-6
        assert rel(z[k + "vol64"], v64.numpy()) <= 1e-12 and rel(z[k + "est64"], e64.numpy()) <= 1e-12
        zeroed = list(z[k + "zeroed"])
        assert len(zeroed) >= 2 and not z[k + "vol"][0, zeroed].any() and int(z[k + "tuple_len"]) == 6


@pytest.mark.parametrize("name", SPLIT)
def test_restatement_reproduces_the_reference_convolutions(name):
    z = load_golden(f"g25_deconv_split_{name}")
    vol, psf, ps = torch.from_numpy(z["vol"]), torch.from_numpy(z["psf"]), [int(v) for v in z["psf_shape"]]
    img2, otf2 = R.fft_conv_split(vol, psf, ps, 2)
    img1 = R.fft_conv_split(vol, otf2, ps, 1, True)[0]
    full = (vol.shape[2] + ps[0], vol.shape[3] + ps[1])
    conv = R.fft_conv(vol, psf, full)[0]
    assert np.array_equal(img2.numpy(), z["img2"]) and np.array_equal(otf2.numpy(), z["otf2"]) and np.array_equal(img1.numpy(), z["img1"])
    assert np.array_equal(conv.numpy(), z["conv"]) and conv.shape[2:] == full
    a64, o64 = R.fft_conv_split(vol, psf, ps, 2, dtype=torch.float64)
    assert rel(z["img2"], a64.numpy()) <= float(z["dev_img2"]) * (1 + 1e-6) < 2e-6
    assert rel(z["otf2"], o64.numpy()) <= float(z["dev_otf"]) * (1 + 1e-6) < 2e-6
    assert rel(z["img2_64"], a64.numpy()) <= 1e-12 and rel(z["otf2_64"], o64.numpy()) <= 1e-12


def test_restatement_shift_is_the_rolls_of_the_reference():
    x = torch.arange(2 * 5 * 6, dtype=torch.float32).reshape(1, 2, 5, 6)
    want = torch.cat([x[:, :, 3:], x[:, :, :3]], 2)
    want = torch.cat([want[..., 3:], want[..., :3]], 3)
    assert torch.equal(R.shift(x), want)
    assert list(R.np_shift_index(5)) == [3, 4, 0, 1, 2] and list(R.np_shift_index(6, 1)) == [4, 5, 0, 1, 2, 3]
    from cwfa_amd import utils as U
    assert torch.equal(U.roll_n(x, 2, 3), torch.cat([x[:, :, 3:], x[:, :, :3]], 2))


def test_psf_selection_and_normalisation_match_the_reference():
    from cwfa_amd import utils as U
    z = load_golden("g25_deconv_psf")
    psf = U.load_PSF(torch.from_numpy(z["raw"]), 4)
    assert np.array_equal(psf.numpy(), z["psf"])
    assert z["otf5"].shape == z["otf"].shape + (2,) and np.array_equal(z["otf5"][..., 0], z["otf"])
    assert np.array_equal(z["otf5"][..., 1], np.conj(z["otf"]))


def test_spectrum_mul_arguments(L, ptr):
    p = ptr
    assert L.cwfa_deconv_spectrum_mul_c64(None, p, p, 1, 8, 1, 0, None) == -1 and b"null" in L.cwfa_last_error()
    assert L.cwfa_deconv_spectrum_mul_c64(p, None, p, 1, 8, 1, 0, None) == -1
    assert L.cwfa_deconv_spectrum_mul_c64(p, p, None, 1, 8, 1, 0, None) == -1
    assert L.cwfa_deconv_spectrum_mul_c64(p, p, p, -1, 8, 1, 0, None) == -2
    assert L.cwfa_deconv_spectrum_mul_c64(p, p, p, 1, -8, 1, 0, None) == -2
    q = ctypes.c_void_p(p.value + 1024)
    assert L.cwfa_deconv_spectrum_mul_c64(p, q, p, 3, 8, 2, 0, None) == -1 and b"neither 1 nor D" in L.cwfa_last_error()
    assert L.cwfa_deconv_spectrum_mul_c64(p, q, q, 3, 8, 3, 0, None) == -1 and b"never written" in L.cwfa_last_error()
    assert L.cwfa_deconv_spectrum_mul_c64(p, q, p, 0, 8, 0, 0, None) == 0 and L.cwfa_deconv_spectrum_mul_c64(p, q, p, 3, 0, 3, 1, None) == 0


def test_project_arguments(L, ptr):
    p, q = ptr, ctypes.c_void_p(ptr.value + 1024)
    assert L.cwfa_deconv_project_f32(None, q, 1, 1, 8, 8, 8, 8, 0, 0, 0, 0, 0, None) == -1 and b"null" in L.cwfa_last_error()
    assert L.cwfa_deconv_project_f32(p, None, 1, 1, 8, 8, 8, 8, 0, 0, 0, 0, 0, None) == -1
    assert L.cwfa_deconv_project_f32(p, q, 1, -1, 8, 8, 8, 8, 0, 0, 0, 0, 0, None) == -2
    assert L.cwfa_deconv_project_f32(p, q, 1, 1, 8, -8, 8, 8, 0, 0, 0, 0, 0, None) == -2
    assert L.cwfa_deconv_project_f32(p, q, 1, 1, 8, 8, -1, 8, 0, 0, 0, 0, 0, None) == -2
    for win in ((8, 8, 1, 0), (8, 8, 0, 1), (4, 4, 5, 0), (4, 4, 0, 5), (4, 4, -1, 0), (4, 4, 0, -1), (9, 4, 0, 0)):
        assert L.cwfa_deconv_project_f32(p, q, 1, 1, 8, 8, *win, 0, 0, 0, None) == -1 and b"not inside" in L.cwfa_last_error(), win
    assert L.cwfa_deconv_project_f32(p, q, 1, 1, 8, 8, 8, 8, 0, 0, 2, 0, 0, None) == -1 and b"pre" in L.cwfa_last_error()
    assert L.cwfa_deconv_project_f32(p, q, 1, 1, 8, 8, 8, 8, 0, 0, 0, 2, 0, None) == -1 and b"post" in L.cwfa_last_error()
    assert L.cwfa_deconv_project_f32(p, q, 0, 1, 8, 8, 8, 8, 0, 0, 0, 0, 0, None) == 0
    assert L.cwfa_deconv_project_f32(p, q, 1, 1, 8, 8, 0, 8, 0, 0, 1, 1, 1, None) == 0


def test_ratio_clamp_update_select_arguments(L, ptr):
    p, q = ptr, ctypes.c_void_p(ptr.value + 1024)
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.cwfa_deconv_ratio_f32(*args, 8, None) == -1 and b"null" in L.cwfa_last_error()
    assert L.cwfa_deconv_ratio_f32(p, p, p, p, -1, None) == -2 and L.cwfa_deconv_ratio_f32(p, p, p, p, 0, None) == 0
    for args in ((None, 8, p, p), (p, 8, None, p), (p, 8, p, None)):
        assert L.cwfa_deconv_clamp_f32(*args, 10.0, None) == -1 and b"null" in L.cwfa_last_error()
    assert L.cwfa_deconv_clamp_f32(p, -8, p, p, 10.0, None) == -2 and L.cwfa_deconv_clamp_f32(p, 0, p, p, 10.0, None) == 0
    assert L.cwfa_deconv_update_f32(None, q, 1, 8, 4, 2, None) == -1 and L.cwfa_deconv_update_f32(p, None, 1, 8, 4, 2, None) == -1
    assert L.cwfa_deconv_update_f32(p, q, -1, 8, 4, 2, None) == -2 and L.cwfa_deconv_update_f32(p, q, 1, 8, -4, 2, None) == -2
    assert L.cwfa_deconv_update_f32(p, q, 1, 8, 4, 5, None) == -1 and b"not inside" in L.cwfa_last_error()
    assert L.cwfa_deconv_update_f32(p, q, 1, 8, 4, -1, None) == -1 and L.cwfa_deconv_update_f32(p, q, 1, 8, 9, 0, None) == -1
    assert L.cwfa_deconv_update_f32(p, p, 1, 8, 4, 2, None) == -1 and b"same tensor" in L.cwfa_last_error()
    assert L.cwfa_deconv_update_f32(p, q, 0, 8, 4, 2, None) == 0 and L.cwfa_deconv_update_f32(p, q, 1, 8, 0, 2, None) == 0
    assert L.cwfa_select_nonzero_f32(p, 1, 8, 8, 0, None, p, p, None) == -1 and b"cwfa_select_nonzero_f32: null" in L.cwfa_last_error()
    assert L.cwfa_select_nonzero_f32(None, 1, 8, 8, 0, p, p, p, None) == -1
    assert L.cwfa_select_nonzero_f32(p, 1, -8, 8, 0, p, p, p, None) == -2
    assert L.cwfa_select_nonzero_f32(p, 1, 8, 8, 8, p, p, p, None) == -1 and b"not below" in L.cwfa_last_error()
    assert L.cwfa_select_nonzero_f32(p, 1, 8, 8, -2, p, p, p, None) == -1 and L.cwfa_select_nonzero_f32(p, 0, 8, 8, 0, p, p, p, None) == 0
    assert L.cwfa_select_positive_f32(p, 1, 8, 8, 8, p, p, p, None) == -1 and b"cwfa_select_positive_f32: k = 8" in L.cwfa_last_error()


def test_mirrors_refuse_what_they_cannot_run():
    from cwfa_amd import utils as U
    otf = torch.zeros(1, 3, 36, 19, dtype=torch.complex64)
    img = torch.ones(1, 1, 24, 24)
    with pytest.raises(NotImplementedError, match="verbose"):
        U.XLFMDeconv(otf, img, 2, ObjSize=[12, 12], verbose=True)
    with pytest.raises(NotImplementedError, match="calc_max"):
        U.load_PSF_OTF(torch.ones(1, 9, 24, 24), [12, 12, 4], calc_max=True)
    with pytest.raises(NotImplementedError, match="file"):
        U.load_PSF("psf.mat", 4)
    with pytest.raises(ValueError, match="full size 37 is odd"):
        U.XLFMDeconv(torch.zeros(1, 3, 37, 19, dtype=torch.complex64), img, 2, ObjSize=[13, 13])
    with pytest.raises(ValueError, match="object size 13"):
        U.XLFMDeconv(otf, img, 2, ObjSize=[13, 13])
    with pytest.raises(ValueError, match="image size 23"):
        U.XLFMDeconv(otf, torch.ones(1, 1, 23, 23), 2, ObjSize=[12, 12])
    with pytest.raises(ValueError, match="not square"):
        U.XLFMDeconv(otf, img, 2, ObjSize=[12, 14])
    with pytest.raises(ValueError, match="not square"):
        U.XLFMDeconv(otf, torch.ones(1, 1, 24, 22), 2, ObjSize=[12, 12])
    with pytest.raises(ValueError, match="full width 37 is odd"):
        U.fft_conv(torch.ones(1, 2, 12, 13), torch.ones(1, 2, 24, 24), [36, 37])
    with pytest.raises(ValueError, match="full width 37 is odd"):
        U.fft_conv_split(torch.ones(1, 2, 12, 13), torch.ones(1, 2, 24, 24), [24, 24], 1)
    with pytest.raises(TypeError, match="real"):
        U.batch_fftshift2d_real(otf)
    # what passes the size rules still needs the device: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.XLFMDeconv(otf, img, 2, ObjSize=[12, 12])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.fft_conv_split(torch.ones(1, 2, 13, 12), torch.ones(1, 2, 24, 24), [24, 24], 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.batch_fftshift2d_real(torch.ones(1, 1, 4, 4))


def test_install_registers_utils_only_when_asked():
    import sys

    import cwfa_amd
    saved = {k: sys.modules.get(k) for k in ("utils", "FrEIA", "FrEIA.framework", "FrEIA.modules", "INN_utils", "networks", "unet")}
    try:
        sys.modules.pop("utils", None)
        cwfa_amd.install()
        assert "utils" not in sys.modules
        cwfa_amd.install(utils=True)
        ns = {}
        exec("from utils import *", ns)
        for name in ("roll_n", "batch_fftshift2d_real", "fft_conv", "fft_conv_split", "load_PSF", "load_PSF_OTF", "XLFMDeconv"):
            assert callable(ns[name]), name
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
