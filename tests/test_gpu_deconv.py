"""GPU: the Richardson-Lucy deconvolution.

Each kernel of csrc/deconv_ops.hip alone against a numpy float64 restatement, with the bound its arithmetic gives:
  spectrum_mul   per component 2^-22 (|a_re b_re| + |a_im b_im|) (real part; the imaginary part likewise): two rounded products and
                 one rounded sum, the library is built with -ffp-contract=off;
  project        the float64 sum rounded to fp32, within D 2^-24 sum|terms| (D - 1 rounded additions in a fixed order and the
                 rounding of the yardstick; the value accumulated onto counts as a term);
  ratio, clamp, update, select_nonzero   exact (one IEEE operation per element, or a selection).
Then XLFMDeconv, fft_conv_split, fft_conv and load_PSF_OTF on the fixtures recorded from the reference
(tests/golden/g25_deconv_*.npz): max|gpu - f64| <= 8 dev_ref max|f64|, dev_ref the reference's own fp32 distance from the float64
restatement; the margin 8 covers rocFFT's factorisation, the sequential depth sum and the fused product, each of that order."""
import itertools

import numpy as np
import pytest
import torch

import deconv_ref as R
from conftest import load_golden
from test_deconv_cpu import RL, SPLIT, rel, rl

pytestmark = pytest.mark.gpu
MARGIN = 8.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def crandn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape", [(3, 10, 6), (5, 46, 24), (3, 5, 7)])
def test_spectrum_mul(shape):
    from cwfa_amd import ops
    rng = np.random.default_rng(sum(shape))
    D, n = shape[0], shape[1] * shape[2]
    otf_h = crandn(rng, shape)
    for conj, bcast, inplace, misaligned in itertools.product((False, True), (False, True), (False, True), (False, True)):
        if inplace and bcast:
            continue
        a_h = crandn(rng, (1,) + shape[1:] if bcast else shape)
        if misaligned:                                       # every base pointer one complex value past a 16-byte boundary
            ab, ob, rb = (torch.zeros(1 + k, dtype=torch.complex64, device="cuda") for k in (a_h.size, D * n, D * n))
            a, otf, out = ab[1:].view(a_h.shape), ob[1:].view(shape), rb[1:].view(shape)
            a.copy_(dev(a_h)), otf.copy_(dev(otf_h))
            assert a.data_ptr() % 16 == 8 and otf.data_ptr() % 16 == 8
        else:
            a, otf, out = dev(a_h), dev(otf_h), torch.zeros(shape, dtype=torch.complex64, device="cuda")
        got = host(ops.deconv_spectrum_mul(a, otf, conj=conj, out=a if inplace else out))
        assert np.array_equal(host(otf).view(np.uint32), otf_h.view(np.uint32)), "otf is never written"
        ar, ai = a_h.real.astype(np.float64), a_h.imag.astype(np.float64)
        br, bi = otf_h.real.astype(np.float64), otf_h.imag.astype(np.float64) * (-1 if conj else 1)
        err_re, err_im = np.abs(got.real - (ar * br - ai * bi)), np.abs(got.imag - (ar * bi + ai * br))
        what = (shape, conj, bcast, inplace, misaligned)
        assert (err_re <= 2.0 ** -22 * (np.abs(ar * br) + np.abs(ai * bi))).all(), what
        assert (err_im <= 2.0 ** -22 * (np.abs(ar * bi) + np.abs(ai * br))).all(), what
    assert host(ops.deconv_spectrum_mul(dev(otf_h), dev(otf_h))).shape == shape          # out defaults to a new tensor


@pytest.mark.parametrize("H,W,window", [(37, 38, None), (37, 38, (6, 7, 24, 24)), (46, 46, None), (46, 46, (6, 7, 24, 24)),
                                        (40, 48, None), (40, 48, (6, 8, 24, 24))])
@pytest.mark.parametrize("D", [1, 5])
def test_project(H, W, window, D):
    from cwfa_amd import ops
    rng = np.random.default_rng(H * W + D)
    N = 2
    p_h = rng.standard_normal((N, D, H, W)).astype(np.float32)
    Ho, Wo = (H, W) if window is None else window[2:]
    prev_h = rng.standard_normal((N, 1, Ho, Wo)).astype(np.float32)
    p = dev(p_h)
    for pre, post, acc in itertools.product((None, "relu"), (None, "abs"), (False, True)):
        out = dev(prev_h)
        ret = ops.deconv_project(p, out=out, window=window, pre=pre, post=post, accumulate=acc)
        assert ret.data_ptr() == out.data_ptr()
        s, mag = R.np_project(p_h, window, pre, post)
        if acc:
            s, mag = s + prev_h[:, 0], mag + np.abs(prev_h[:, 0])
        got = host(out)[:, 0].astype(np.float64)
        err = np.abs(got - s.astype(np.float32).astype(np.float64))
        assert (err <= D * 2.0 ** -24 * mag).all(), (H, W, window, D, pre, post, acc, float((err / mag).max()))
    assert np.array_equal(bits(host(p)), bits(p_h))
    if window is None and D == 1:                                                        # the plain shift is exact
        from cwfa_amd import utils as U
        x = p[:, :1].reshape(1, N, H, W).contiguous()
        assert torch.equal(U.batch_fftshift2d_real(x), R.shift(x))


@pytest.mark.parametrize("n", [1003, 4096])
def test_ratio_and_its_flag(n):
    from cwfa_amd import ops
    rng = np.random.default_rng(n)
    img = rng.standard_normal(n).astype(np.float32) * 3
    est = np.abs(rng.standard_normal(n)).astype(np.float32)
    img[::7], est[::5] = 0.0, 0.0
    eps = np.float32(1e-8)

    def run(img_h, est_h):
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = ops.deconv_ratio(dev(img_h), dev(est_h), torch.empty(n, device="cuda"), flag)
        with np.errstate(all="ignore"):
            want = img_h / (est_h + eps)
        got, nan = host(out), np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan])), "one IEEE division per element"
        return int(flag.item())

    assert (img < 0).any() and (img == 0).any() and run(img, est) == 0, "zeros and negatives are no reason to stop"
    for bad in (np.inf, -np.inf, np.nan):
        for at in (0, n // 2 + 1, n - 1):
            x = img.copy()
            x[at] = bad
            assert run(x, est) == 1, (bad, at)
    e = est.copy()
    x = img.copy()
    e[n - 2], x[n - 2] = -eps, 0.0                                                     # 0 / 0: the ratio itself is NaN
    assert run(x, e) == 1


@pytest.mark.parametrize("n", [1003, 4096])
def test_clamp_reads_its_bound_from_the_device(n):
    from cwfa_amd import ops
    rng = np.random.default_rng(n + 1)
    x_h = (rng.standard_normal(n) * 20).astype(np.float32)
    x_h[3], x_h[n - 1] = np.nan, np.inf
    for med in (0.37, -0.2):
        median, count = dev(np.array([med], dtype=np.float32)), dev(np.array([5], dtype=np.int64))
        got = host(ops.deconv_clamp(dev(x_h), median, count, 10))
        hi = np.float32(med) * np.float32(10)
        want = np.minimum(np.maximum(x_h, np.float32(0)), hi)                           # numpy keeps NaN, like torch.clamp_
        assert np.isnan(got[3]) and np.array_equal(bits(got[~np.isnan(x_h)]), bits(want[~np.isnan(x_h)]))
    none = dev(np.array([0], dtype=np.int64))
    got = host(ops.deconv_clamp(dev(x_h), dev(np.array([np.nan], dtype=np.float32)), none, 10))
    assert np.array_equal(bits(got), bits(x_h)), "count == 0 leaves the plane alone"


@pytest.mark.parametrize("F,obj", [(46, 14), (48, 16), (37, 13)])
def test_update_touches_the_window_only(F, obj):
    from cwfa_amd import ops
    rng = np.random.default_rng(F)
    D, po = 3, (F - obj) // 2
    o_h = np.zeros((1, D, F, F), dtype=np.float32)
    o_h[:, :, po:po + obj, po:po + obj] = rng.standard_normal((1, D, obj, obj)).astype(np.float32)
    b_h = rng.standard_normal((1, D, F, F)).astype(np.float32)
    idx = R.np_shift_index(F)
    inside = np.zeros((F, F), dtype=bool)
    inside[np.ix_(idx[po:po + obj], idx[po:po + obj])] = True
    b_h[:, :, ~inside] = np.nan                                                          # whatever lies outside the window is not used
    o = ops.deconv_update(dev(o_h), dev(b_h), obj, po)
    got = host(o)
    want = o_h[:, :, po:po + obj, po:po + obj] * b_h[:, :, idx][:, :, :, idx][:, :, po:po + obj, po:po + obj]
    assert np.array_equal(bits(got[:, :, po:po + obj, po:po + obj]), bits(want))
    border = np.ones((F, F), dtype=bool)
    border[po:po + obj, po:po + obj] = False
    assert (bits(got[:, :, border]) == 0).all(), "the border stays exactly +0.0"


def test_select_nonzero():
    from cwfa_amd import ops
    rng = np.random.default_rng(25)
    x = (rng.standard_normal(1000) * 5).astype(np.float32)
    x[::9], x[1::9] = 0.0, -0.0
    x[2::50] = x[2]                                                                      # ties
    x[3::50] = -np.abs(x[3])
    srt = np.sort(x[x != 0])
    assert (srt < 0).sum() > 100 and (srt > 0).sum() > 100
    d = dev(x)
    for k in [0, len(srt) - 1] + [len(srt) * q // 10 for q in range(1, 10)]:
        val, cnt = ops.select_nonzero(d, k)
        assert int(cnt.item()) == len(srt) and bits(host(val))[0] == bits(srt[k:k + 1])[0], k
    val, cnt = ops.select_nonzero(d)
    want = torch.from_numpy(x)[torch.from_numpy(x) != 0].median()
    assert float(val.item()) == float(want) == float(R.np_select_nonzero(x)[0])
    val, cnt = ops.select_nonzero(dev(np.array([0.0, -0.0, 0.0, -0.0, 0.0], dtype=np.float32)))
    assert int(cnt.item()) == 0 and np.isnan(float(val.item()))
    for arr in ([-3.0, 0.0, -1.0, -2.0], [-1.0, 2.0], [4.0, 0.0, -0.0, 4.0, 4.0], [-7.5]):
        a = np.array(arr, dtype=np.float32)
        val, cnt = ops.select_nonzero(dev(a))
        assert (float(val.item()), int(cnt.item())) == (float(torch.from_numpy(a)[torch.from_numpy(a) != 0].median()), int((a != 0).sum())), arr
    pv, pc = ops.select_positive(d.reshape(1, 1, 1, -1))                                 # the positive selection is what it was
    pos = np.sort(x[x > 0])
    assert int(pc.item()) == len(pos) and float(pv.item()) == float(pos[(len(pos) - 1) // 2])


def test_offsets_beyond_2_31_elements():
    """The kernels index with 64 bits: a spectrum of 2^30 + 8 complex values (2^31 + 16 floats) and a stack of 130 planes of
    4096 x 4096 (2^31 + 2^25 floats), zero except at the far end, where a 32-bit offset would wrap to the front."""
    from cwfa_amd import ops
    rng = np.random.default_rng(31)
    n, tail = 2 ** 30 + 8, 1024
    a = torch.zeros(1, 1, n, dtype=torch.complex64, device="cuda")
    otf = torch.zeros(1, 1, n, dtype=torch.complex64, device="cuda")
    a_h, o_h = crandn(rng, tail), crandn(rng, tail)
    a[0, 0, -tail:], otf[0, 0, -tail:] = dev(a_h), dev(o_h)
    ops.deconv_spectrum_mul(a, otf, conj=True, out=a)
    want = a_h.astype(np.complex128) * np.conj(o_h.astype(np.complex128))
    got = host(a[0, 0, -tail:])
    assert np.abs(got - want).max() <= 2.0 ** -21 * np.abs(want).max() and np.abs(want).max() > 1
    assert not a[0, 0, :tail].any(), "nothing wrapped to the front"
    del a, otf
    D, S = 130, 4096
    p = torch.zeros(1, D, S, S, device="cuda")
    last = torch.randn(S, S, device="cuda")
    p[0, D - 1] = last
    out = ops.deconv_project(p)
    assert torch.equal(out[0, 0], R.shift(last[None, None])[0, 0])
    obj_pad = p
    obj_pad[0, D - 1] = 0
    obj_pad[0, D - 1, 1024:3072, 1024:3072] = 2.0
    b = torch.zeros(1, D, S, S, device="cuda")
    b[0, D - 1] = last
    ops.deconv_update(obj_pad, b, 2048, 1024)
    assert torch.equal(obj_pad[0, D - 1, 1024:3072, 1024:3072], 2.0 * R.shift(last[None, None])[0, 0, 1024:3072, 1024:3072])
    assert not obj_pad[0, :D - 1].any()


# ------------------------------------------------------------------------------------------------ the mirrors on the fixtures
def deconv_args(z):
    return dict(ObjSize=[int(v) for v in z["ObjSize"]], PSFShape=[int(v) for v in z["PSFShape"]], ROIsize=[int(v) for v in z["ROIsize"]],
                update_median_limit_multiplier=int(z["mult"]))


@pytest.mark.parametrize("name,ns", [(n, s) for n in RL for s in RL[n]])
def test_xlfm_deconv_matches_the_reference(name, ns):
    from cwfa_amd import utils as U
    z = rl(name)
    k = f"n{ns}/"
    OTF, img = dev(z["OTF"]), dev(z["img"])
    out = U.XLFMDeconv(OTF, img, int(z["nIt"]), n_split_fourier=ns, **deconv_args(z))
    again = U.XLFMDeconv(OTF, img, int(z["nIt"]), n_split_fourier=ns, **deconv_args(z))
    assert len(out) == int(z[k + "tuple_len"]) == 6 and out[1] == 0 and out[3] == []
    assert out[4] == list(z[k + "padSize"]) and out[5] == list(z[k + "padSizeImg"])
    vol, est = host(out[0]), host(out[2])
    assert vol.shape == z[k + "vol"].shape and est.shape == z[k + "est"].shape
    e_vol, e_est = rel(vol, z[k + "vol64"]), rel(est, z[k + "est64"])
    print(f"{name} n_split_fourier={ns}: volume {e_vol:.3e} (dev_ref {float(z[k + 'dev_vol']):.3e}), "
          f"estimate {e_est:.3e} (dev_ref {float(z[k + 'dev_est']):.3e})")
    assert e_vol <= MARGIN * float(z[k + "dev_vol"]) and e_est <= MARGIN * float(z[k + "dev_est"])
    assert (bits(vol[0, list(z[k + "zeroed"])]) == 0).all()
    assert np.array_equal(bits(vol), bits(host(again[0]))) and np.array_equal(bits(est), bits(host(again[2]))), "two calls, one result"
    assert np.array_equal(host(img), z["img"]) and np.array_equal(host(OTF), z["OTF"]), "inputs are left alone"


@pytest.mark.parametrize("name", SPLIT)
def test_fft_conv_split_and_fft_conv_match_the_reference(name):
    from cwfa_amd import utils as U
    z = load_golden(f"g25_deconv_split_{name}")
    vol, psf, ps = dev(z["vol"]), dev(z["psf"]), torch.tensor(z["psf_shape"])
    img2, otf2 = U.fft_conv_split(vol, psf, ps, 2)
    assert img2.shape == z["img2"].shape and otf2.shape == z["otf2"].shape and otf2.dtype == torch.complex64
    assert rel(host(img2), z["img2_64"]) <= MARGIN * float(z["dev_img2"])
    assert rel(host(otf2), z["otf2_64"]) <= MARGIN * float(z["dev_otf"])
    img1 = U.fft_conv_split(vol, dev(z["otf2"]), ps, 1, B_precomputed=True)
    assert torch.is_tensor(img1) and rel(host(img1), z["img1_64"]) <= MARGIN * float(z["dev_img1"])
    full = [vol.shape[2] + int(ps[0]), vol.shape[3] + int(ps[1])]
    conv, otf = U.fft_conv(vol, psf, torch.tensor(full))
    assert list(conv.shape[2:]) == full and rel(host(conv), z["conv64"]) <= MARGIN * float(z["dev_conv"])
    assert rel(host(otf), z["otf2_64"]) <= MARGIN * float(z["dev_otf"])
    conv_pre = U.fft_conv(vol, dev(z["otf2"]), torch.tensor(full), B_precomputed=True)
    assert torch.is_tensor(conv_pre) and rel(host(conv_pre), z["conv64"]) <= MARGIN * float(z["dev_conv"])
    assert np.array_equal(host(vol), z["vol"]) and np.array_equal(host(psf), z["psf"])


def test_load_psf_otf_matches_the_reference():
    from cwfa_amd import utils as U
    z = load_golden("g25_deconv_psf")
    raw = dev(z["raw"])
    # per depth a sum of 24 x 24 positive fp32 values (any order: <= 576 2^-24 relative, far less for a tree) and one division
    assert rel(host(U.load_PSF(raw, 4)), z["psf"].astype(np.float64)) <= 2.0 ** -20
    otf, shape = U.load_PSF_OTF(raw, [int(v) for v in z["vol_size"]], n_split=2)
    assert list(shape) == list(z["psf_shape"]) and otf.shape == z["otf"].shape
    assert rel(host(otf), z["otf64"]) <= MARGIN * float(z["dev_otf"])
    otf5, _ = U.load_PSF_OTF(raw, [int(v) for v in z["vol_size"]], n_split=2, compute_OTF=True)
    assert otf5.shape == z["otf5"].shape and torch.equal(otf5[..., 0], otf) and torch.equal(otf5[..., 1], otf.conj())
    with pytest.raises(NotImplementedError):
        U.load_PSF_OTF(raw, [12, 12, 4], calc_max=True)


# ------------------------------------------------------------------------------------------------ control flow
def test_zero_image_returns_the_four_tuple():
    from cwfa_amd import utils as U
    z = rl("i")
    img = torch.zeros_like(dev(z["img"]))
    out = U.XLFMDeconv(dev(z["OTF"]), img, 3, **deconv_args(z))
    D, obj = z["OTF"].shape[1], int(z["ObjSize"][0])
    assert len(out) == 4 and out[3] == [] and out[2] is img
    assert out[0].shape == (1, D, obj, obj) and not out[0].any()
    assert out[1].device.type == "cpu" and out[1].shape == (1, 1, obj + 2 * D + 2, obj + 2 * D + 2)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_pixel_stops_before_the_first_update(bad, capsys):
    from cwfa_amd import utils as U
    z = rl("i")
    img_h = z["img"].copy()
    img_h[0, 0, 10, 11] = bad
    out = U.XLFMDeconv(dev(z["OTF"]), dev(img_h), 3, **deconv_args(z))
    assert "nan found at it: 1" in capsys.readouterr().out and len(out) == 6
    want = R.xlfm_deconv(torch.from_numpy(z["OTF"]), torch.from_numpy(img_h), 3, [int(v) for v in z["ObjSize"]], [int(v) for v in z["ROIsize"]])
    assert want[4] == 0 and np.array_equal(host(out[0]), want[0].numpy())
    vol = host(out[0])
    zeroed = list(z["n1/zeroed"])
    kept = [d for d in range(vol.shape[1]) if d not in zeroed]
    assert (vol[0, zeroed] == 0).all() and (vol[0, kept] == 1).all()
    assert np.array_equal(np.isnan(host(out[2])), np.isnan(want[1].numpy())) and np.isnan(host(out[2])).sum() == 1


def test_refusals_on_the_device():
    from cwfa_amd import utils as U
    z = rl("i")
    with pytest.raises(NotImplementedError, match="verbose"):
        U.XLFMDeconv(dev(z["OTF"]), dev(z["img"]), 2, verbose=True, **deconv_args(z))
    with pytest.raises(ValueError, match="37"):
        U.XLFMDeconv(torch.zeros(1, 3, 37, 19, dtype=torch.complex64, device="cuda"), dev(z["img"]), 2, ObjSize=[13, 13])
    with pytest.raises(ValueError, match="full width 37 is odd"):
        U.fft_conv_split(torch.ones(1, 2, 12, 13, device="cuda"), torch.ones(1, 2, 24, 24, device="cuda"), [24, 24], 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.XLFMDeconv(torch.from_numpy(z["OTF"]), torch.from_numpy(z["img"]), 2, **deconv_args(z))
