"""GPU: shot-noise simulation -- cwfa_rand_poisson_f32 / ops.rand_poisson against the float64 restatement
of poisson_ref.py element by element, its bitwise properties, the dataset augmentation, XLFMForward and simulate_XLFM_image.

Parity.  The kernel and the restatement evaluate the same float64 expressions on the same Philox words; sqrt, division, floor and
the products are correctly rounded on both sides (the library is built with -ffp-contract=off), so they can differ only where the
device's log / lgamma / exp round differently from numpy's AND a comparison sits within that rounding: at most MAX_MISMATCH = 2
elements per case (about 3e-5 of the largest), and each of them must be the proposal of a neighbouring PTRS attempt or k +- 1,
never an arbitrary value (observed on the MI355X: 0 mismatches in every case).  test_poisson_cpu.py shows the restatement itself loses nothing to float64 (0 differences to longdouble).

XLFMForward: the bound of test_gpu_deconv.py for ImgEst, max|gpu - f64| <= 8 dev_ref max|f64|, dev_ref from the fixture."""
import ctypes as C

import numpy as np
import pytest
import torch

import deconv_ref as R
import poisson_ref as P
import sampler_ref as S
from conftest import load_golden

pytestmark = pytest.mark.gpu
SEED = 0x5EED_C0FFEE
MAX_MISMATCH = 2
MARGIN = 8.0
PLANTED = [0.0, 9.999, 10.0, float(np.nextafter(np.float32(10), np.float32(-np.inf))), float(np.nextafter(np.float32(10), np.float32(np.inf))),
           2.0 ** 24, 2.0 ** 30]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def assert_parity(got, lam, seed, stream=0, sample_offset=0, n_samples=None, pre=None, post=None, what=""):
    """got (numpy) against the restatement; returns the number of mismatches (<= MAX_MISMATCH, each one explained)."""
    want, att = P.rand_poisson(lam, seed, stream, sample_offset, n_samples, pre, post, return_attempts=True)
    assert got.shape == want.shape and got.dtype == np.float32
    N = want.shape[0]
    g, w, a = got.reshape(N, -1), want.reshape(N, -1), att.reshape(N, -1)
    bad = np.argwhere(~same(g, w))
    print(f"{what}: {len(bad)} of {w.size} elements differ from the restatement")
    assert len(bad) <= MAX_MISMATCH
    lam32 = np.asarray(lam, dtype=np.float32)
    rates = np.broadcast_to(lam32.reshape(1, -1), w.shape) if n_samples is not None else lam32.reshape(N, -1)
    pre_v = np.ones(N, np.float32) if pre is None else np.broadcast_to(np.asarray(pre, np.float32), (N,))
    post_v = np.ones(N, np.float32) if post is None else np.broadcast_to(np.asarray(post, np.float32), (N,))
    for s, e in bad:
        rate = np.float32(rates[s, e] * pre_v[s])
        k = float(P.draw_plane([rate], sample_offset + s, seed, stream, e0=e)[0][0])
        allowed = {k - 1, k + 1}
        if a[s, e] >= 1:                                                   # PTRS: the proposals of the attempts next to the accepted one
            j = int(a[s, e]) - 1
            allowed |= {P.ptrs_proposal(rate, e, jj, sample_offset + s, seed, stream) for jj in (j - 1, j + 1) if 0 <= jj < 64}
        allowed = {float(np.float32(np.float32(v) * post_v[s])) for v in allowed}
        print(f"  sample {s} element {e}: rate {rate!r}, restatement {w[s, e]!r} after {a[s, e]} attempts, device {g[s, e]!r}")
        assert float(g[s, e]) in allowed, "not a neighbouring draw"
    return len(bad)


def planted_rates(n, seed):
    lam = P.mixed_rates(n, np.random.default_rng(seed))
    if n >= 64:
        lam[np.arange(len(PLANTED)) * 7 + 3] = np.array(PLANTED, dtype=np.float32)
    return lam


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("n", [1, 4099, (1 << 16) + 3])
def test_one_sample_matches_the_restatement(n):
    from cwfa_amd import ops
    lam = planted_rates(n, 11)[None]
    got = host(ops.rand_poisson(dev(lam), SEED))
    assert_parity(got, lam, SEED, what=f"n = {n}")
    k = got[0]
    ok = ~np.isnan(k)
    assert ok.all() and np.array_equal(k, np.rint(k)) and k.min() >= 0
    if n >= 64:
        assert k[3] == 0 and abs(k[3 + 7 * 6] - 2.0 ** 30) < 12 * 2.0 ** 15


def test_samples_with_their_own_rates_and_with_a_shared_plane():
    from cwfa_amd import ops
    lam = np.stack([planted_rates(2053, 20 + i) for i in range(3)])
    got = host(ops.rand_poisson(dev(lam), SEED, stream=4, sample_offset=9))
    assert_parity(got, lam, SEED, 4, 9, what="N = 3, own rates")
    plane = planted_rates(3001, 31).reshape(1, 3001)
    got = host(ops.rand_poisson(dev(plane), SEED, n_samples=5, sample_offset=2))
    assert got.shape == (5, 1, 3001)
    assert_parity(got, plane, SEED, 0, 2, n_samples=5, what="N = 5, one shared plane")
    assert (got[0] != got[1]).mean() > 0.5, "samples of a shared plane are independent draws"


# ------------------------------------------------------------------------------------------------ bitwise properties
def test_bitwise_properties():
    from cwfa_amd import _lib, ops
    N, n = 5, 3001
    lam = dev(np.stack([planted_rates(n, 40 + i) for i in range(N)]))
    a = ops.rand_poisson(lam, SEED, stream=1, sample_offset=3)
    b = ops.rand_poisson(lam, SEED, stream=1, sample_offset=3)
    assert np.array_equal(bits(host(a)), bits(host(b))), "two calls, one result"
    parts = torch.cat([ops.rand_poisson(lam[:2], SEED, stream=1, sample_offset=3), ops.rand_poisson(lam[2:], SEED, stream=1, sample_offset=5)])
    assert np.array_equal(bits(host(a)), bits(host(parts))), "[0, N) is [0, 2) followed by [2, N)"
    assert (host(a) != host(ops.rand_poisson(lam, SEED, stream=2, sample_offset=3))).mean() > 0.5
    assert (host(a) != host(ops.rand_poisson(lam, SEED + 1, stream=1, sample_offset=3))).mean() > 0.5
    # in place, and into a given tensor
    work = lam.clone()
    ret = ops.rand_poisson(work, SEED, stream=1, sample_offset=3, out=work)
    assert ret is work and np.array_equal(bits(host(work)), bits(host(a)))
    given = torch.full_like(lam, -7.0)
    ops.rand_poisson(lam, SEED, stream=1, sample_offset=3, out=given)
    assert np.array_equal(bits(host(given)), bits(host(a)))
    # a sample stride above n leaves the gap untouched (the C entry point; ops always passes n)
    gap = 13
    wide = torch.full((N, n + gap), -3.0, device="cuda")
    rc = _lib.lib().cwfa_rand_poisson_f32(C.c_void_p(wide.data_ptr()), C.c_void_p(lam.data_ptr()), N, n, n, n + gap, None, None,
                                          C.c_uint64(SEED), C.c_uint32(1), C.c_uint32(3), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert np.array_equal(bits(host(wide[:, :n])), bits(host(a))) and (host(wide[:, n:]) == -3.0).all()
    # the refusals of the entry point: strides below a sample, in place across different strides, more than 2^52 elements
    ptr, st = C.c_void_p(wide.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib()
    assert L.cwfa_rand_poisson_f32(ptr, C.c_void_p(lam.data_ptr()), N, n, n, n - 1, None, None, 0, 0, 0, st) != 0
    assert L.cwfa_rand_poisson_f32(ptr, ptr, N, n, 0, n + gap, None, None, 0, 0, 0, st) != 0
    assert L.cwfa_rand_poisson_f32(ptr, C.c_void_p(lam.data_ptr()), 1, (1 << 52) + 1, 0, 0, None, None, 0, 0, 0, st) != 0
    assert L.cwfa_rand_poisson_f32(None, C.c_void_p(lam.data_ptr()), 1, n, n, n, None, None, 0, 0, 0, st) != 0


# ------------------------------------------------------------------------------------------------ scaling and the NaN contract
def test_pre_and_post():
    from cwfa_amd import ops
    N, n = 3, 2053
    lam_h = np.stack([P.mixed_rates(n, np.random.default_rng(50 + i)) for i in range(N)])
    lam = dev(lam_h)
    pre_h, post_h = np.array([0.37, 2.5, 1.0], dtype=np.float32), np.array([3.0, 0.1, 7.25], dtype=np.float32)
    got = ops.rand_poisson(lam, SEED, pre=dev(pre_h), post=dev(post_h))
    # the unscaled draw at fl32(lam * pre), times post: bitwise, both by the device
    plain = ops.rand_poisson(dev(lam_h * pre_h[:, None]), SEED)
    assert np.array_equal(bits(host(got)), bits(host(plain) * post_h[:, None]))
    assert_parity(host(got), lam_h, SEED, pre=pre_h, post=post_h, what="pre / post tensors")
    # numbers
    num = ops.rand_poisson(lam, SEED, pre=0.37, post=3.0)
    assert np.array_equal(bits(host(num[0])), bits(host(got[0])))
    assert_parity(host(num), lam_h, SEED, pre=0.37, post=3.0, what="pre / post numbers")
    only_post = ops.rand_poisson(lam, SEED, post=0.5)
    assert np.array_equal(bits(host(only_post)), bits(host(ops.rand_poisson(lam, SEED)) * np.float32(0.5)))
    zero = ops.rand_poisson(lam, SEED, pre=0.0, post=dev(post_h))
    assert not host(zero).any()


def test_the_nan_contract():
    from cwfa_amd import ops
    lam = np.array([[0.0, -0.0, -1.0, np.nan, 2.0 ** 30, np.nextafter(np.float32(2.0 ** 30), np.float32(np.inf)), np.inf, -np.inf, 1e-30,
                     5.0, 50.0, -1e-30]], dtype=np.float32)
    k = host(ops.rand_poisson(dev(lam), SEED))[0]
    assert np.isnan(k[[2, 3, 5, 6, 7, 11]]).all()
    assert k[0] == 0 and k[1] == 0 and k[8] == 0 and not np.isnan(k[[4, 9, 10]]).any()
    assert_parity(k[None], lam, SEED, what="edges")
    # a bad rate does not disturb its neighbours, and pre can make a rate bad
    k2 = host(ops.rand_poisson(dev(lam), SEED, pre=-1.0))[0]
    assert np.isnan(k2[[4, 9, 10, 3, 6, 7]]).all() and k2[0] == 0 and k2[1] == 0


def test_refusals_and_empty_input(monkeypatch):
    from cwfa_amd import _lib, ops
    lam = torch.ones(3, 8, device="cuda")
    with pytest.raises(ValueError):
        ops.rand_poisson(lam.cpu(), 1)
    with pytest.raises(ValueError):
        ops.rand_poisson(lam.double(), 1)
    with pytest.raises(ValueError):
        ops.rand_poisson(lam.t(), 1)
    with pytest.raises(ValueError):
        ops.rand_poisson(lam, 1, pre=torch.ones(2, device="cuda"))
    with pytest.raises(ValueError):
        ops.rand_poisson(lam, 1, post=torch.ones(3, 1, device="cuda"))
    with pytest.raises(ValueError):
        ops.rand_poisson(lam, 1, pre=torch.ones(3))
    with pytest.raises(ValueError):
        ops.rand_poisson(lam, 1, post=torch.ones(3, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.rand_poisson(lam, 1, out=torch.empty(3, 9, device="cuda"))
    with pytest.raises(ValueError):
        ops.rand_poisson(lam, 1, n_samples=2, out=lam)
    with pytest.raises(ValueError):
        ops.rand_poisson(lam, -1)
    with pytest.raises(ValueError):
        ops.rand_poisson(lam, 1, stream=1 << 32)

    def no_launch():
        raise AssertionError("an empty input must not reach the library")
    monkeypatch.setattr(_lib, "lib", no_launch)
    assert tuple(ops.rand_poisson(torch.empty(0, 8, device="cuda"), 1).shape) == (0, 8)
    assert tuple(ops.rand_poisson(torch.empty(3, 0, device="cuda"), 1, pre=2.0).shape) == (3, 0)
    assert tuple(ops.rand_poisson(lam[0], 1, n_samples=0).shape) == (0, 8)


# ------------------------------------------------------------------------------------------------ the dataset augmentation
def shot_stack():
    rng = np.random.default_rng(60)
    views = (rng.random((3, 32, 40)) ** 3 * np.array([900.0, 1.0, 0.02])[:, None, None]).astype(np.float32)
    views[1] = 0.0
    return views


def test_add_random_shot_noise_to_dataset():
    from cwfa_amd import ops
    from cwfa_amd.XLFMDataset import ConcatDataset, XLFMDatasetFull, add_random_shot_noise_to_datasets, shot_noise_scales
    views, rng_range, offset = shot_stack(), [16 ** 2, 48 ** 2], 4
    ds = XLFMDatasetFull(dev(views))
    held = ds.stacked_views
    ds.add_random_shot_noise_to_dataset(rng_range, seed=SEED, sample_offset=offset)
    assert ds.stacked_views is held, "in place"
    got = host(ds.stacked_views)
    # the restatement, fed the pre / post the device forms from the restated maxima and uniforms
    m = views.reshape(3, -1).max(1)
    u = S.uniform(3, 1, SEED, stream=1, sample_offset=offset)[:, 0]
    pre, post = (host(t) for t in shot_noise_scales(dev(m), dev(u), rng_range))
    pre_c, post_c = (t.numpy() for t in shot_noise_scales(torch.from_numpy(m), torch.from_numpy(u), rng_range))
    assert np.array_equal(pre, pre_c) and np.array_equal(post, post_c), "the scales do not depend on the device that formed them"
    assert pre[1] == 0 and post[1] == 0 and 16 ** 2 <= pre[0] * m[0] * (1 + 1e-6) and pre[0] * m[0] <= 48 ** 2 * (1 + 1e-6)
    assert_parity(got, views, SEED, 0, offset, pre=pre, post=post, what="dataset")
    assert not got[1].any(), "the all-zero image stays all zero"
    assert not np.isnan(got).any() and (got[0] != views[0]).mean() > 0.5
    # noise at the chosen power: the scaled counts of image 0 scatter around the clean image like Poisson counts
    z = (got[0] - views[0]) * pre[0] / np.sqrt(np.maximum(views[0] * pre[0], 1e-3))
    sel = views[0] * pre[0] > 20
    assert sel.sum() > 100 and abs(z[sel].std() - 1) < 0.2 and abs(z[sel].mean()) < 0.2
    # split 1 + 2 under ConcatDataset (and as a plain list): the bits of the unsplit stack
    whole = XLFMDatasetFull(dev(views))
    add_random_shot_noise_to_datasets(ConcatDataset(whole), rng_range, seed=SEED)
    first, rest = XLFMDatasetFull(dev(views[:1])), XLFMDatasetFull(dev(views[1:]))
    add_random_shot_noise_to_datasets(ConcatDataset(first, rest), rng_range, seed=SEED)
    assert np.array_equal(bits(host(whole.stacked_views)), np.concatenate([bits(host(first.stacked_views)), bits(host(rest.stacked_views))]))
    listed = [XLFMDatasetFull(dev(views[:2])), XLFMDatasetFull(dev(views[2:]))]
    add_random_shot_noise_to_datasets(listed, rng_range, seed=SEED)
    assert np.array_equal(bits(host(whole.stacked_views)), np.concatenate([bits(host(d.stacked_views)) for d in listed]))
    torch.manual_seed(77)
    a_ = [XLFMDatasetFull(dev(views))]
    add_random_shot_noise_to_datasets(a_, rng_range)
    torch.manual_seed(77)
    b_ = [XLFMDatasetFull(dev(views[:1])), XLFMDatasetFull(dev(views[1:]))]
    add_random_shot_noise_to_datasets(b_, rng_range)
    assert np.array_equal(bits(host(a_[0].stacked_views)), np.concatenate([bits(host(d.stacked_views)) for d in b_])), "seed=None: one seed for all"
    # seed=None: torch's generator governs
    runs = []
    for _ in range(2):
        torch.manual_seed(123)
        d = XLFMDatasetFull(dev(views))
        d.add_random_shot_noise_to_dataset(rng_range)
        runs.append(bits(host(d.stacked_views)))
    torch.manual_seed(124)
    d = XLFMDatasetFull(dev(views))
    d.add_random_shot_noise_to_dataset(rng_range)
    assert np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[0], bits(host(d.stacked_views)))
    with pytest.raises(ValueError):
        XLFMDatasetFull(dev(views[..., None].repeat(2, -1))).add_random_shot_noise_to_dataset(seed=1)


# ------------------------------------------------------------------------------------------------ forward projection
def forward64(z, vol):
    """float64 forward projection [1, 1, F, F] of deconv_ref: the first line of its loop."""
    OTF = torch.from_numpy(z["OTF"]).to(torch.complex128)
    Fs, obj = OTF.shape[2], vol.shape[2]
    pad = torch.nn.functional.pad(torch.from_numpy(vol).double(), 4 * [(Fs - obj) // 2])
    return torch.nn.functional.relu(R.shift(torch.fft.irfft2(torch.fft.rfft2(pad) * OTF))).sum(1).unsqueeze(1).numpy()


@pytest.mark.parametrize("name", ["i", "iii"])
def test_xlfm_forward_matches_the_float64_projection(name):
    from cwfa_amd import utils as U
    z = load_golden(f"g25_deconv_rl_{name}")
    vol_h = np.ascontiguousarray(z["n1/vol"])                              # the recorded reconstruction: a realistic non-negative volume
    OTF, vol = dev(z["OTF"]), dev(vol_h)
    want = forward64(z, vol_h)
    tol = MARGIN * float(z["n1/dev_est"]) * np.abs(want).max()
    full = U.XLFMForward(OTF, vol, ObjSize=[int(v) for v in z["ObjSize"]])
    assert tuple(full.shape) == want.shape
    split = U.XLFMForward(OTF, vol, n_split_fourier=2)
    e1, e2 = np.abs(host(full) - want).max(), np.abs(host(split) - want).max()
    print(f"{name}: |gpu - f64| = {e1:.3e} (n_split_fourier 1), {e2:.3e} (2); bound {tol:.3e}; between the two {np.abs(host(full) - host(split)).max():.3e}")
    assert e1 <= tol and e2 <= tol and np.abs(host(full) - host(split)).max() <= tol
    assert np.abs(want).max() > 0
    # the 5-D form uses OTF[..., 0]
    otf5 = torch.stack([OTF, torch.zeros_like(OTF)], dim=-1)
    assert np.array_equal(bits(host(U.XLFMForward(otf5, vol))), bits(host(full)))
    # img_size: the centred window of the full result, bit for bit; out= is written
    S_img, Fs = int(z["img"].shape[2]), want.shape[2]
    pi = (Fs - S_img) // 2
    out = torch.full((1, 1, S_img, S_img), -1.0, device="cuda")
    win = U.XLFMForward(OTF, vol, img_size=[S_img, S_img], out=out)
    assert win is out and np.array_equal(bits(host(win)), bits(host(full)[:, :, pi:pi + S_img, pi:pi + S_img]))
    win2 = U.XLFMForward(OTF, vol, img_size=S_img, n_split_fourier=2)
    assert np.array_equal(bits(host(win2)), bits(host(split)[:, :, pi:pi + S_img, pi:pi + S_img]))
    assert np.array_equal(host(vol), vol_h) and np.array_equal(host(OTF), z["OTF"]), "inputs are left alone"
    with pytest.raises(ValueError):
        U.XLFMForward(OTF, vol, img_size=S_img + 1)
    with pytest.raises(ValueError):
        U.XLFMForward(OTF, vol[:, :-1])
    with pytest.raises(ValueError):
        U.XLFMForward(OTF, vol, ObjSize=[3, 3])


def test_simulate_xlfm_image():
    from cwfa_amd import ops, utils as U
    z = load_golden("g25_deconv_rl_iii")
    OTF, vol = dev(z["OTF"]), dev(np.ascontiguousarray(z["n1/vol"]))
    S_img = int(z["img"].shape[2])
    kw = dict(img_size=S_img, n_split_fourier=2)
    clean, noisy = U.simulate_XLFM_image(OTF, vol, photons=400.0, background=2.5, seed=SEED, n_samples=3, **kw)
    assert tuple(clean.shape) == (1, 1, S_img, S_img) and tuple(noisy.shape) == (3, 1, S_img, S_img)
    assert np.array_equal(bits(host(clean)), bits(host(U.XLFMForward(OTF, vol, **kw))))
    rate = clean[0] * (400.0 / clean.max()) + 2.5                          # the documented rate, in fp32 on the device
    assert np.array_equal(bits(host(noisy)), bits(host(ops.rand_poisson(rate.contiguous(), SEED, n_samples=3))))
    assert_parity(host(noisy), host(rate), SEED, n_samples=3, what="simulate")
    assert abs(float(rate.max()) - 402.5) < 1e-3
    for s in range(3):
        one = U.simulate_XLFM_image(OTF, vol, photons=400.0, background=2.5, seed=SEED, sample_offset=s, **kw)[1]
        assert np.array_equal(bits(host(one[0])), bits(host(noisy[s])))
    # photons=None: the clean image is in photon units already
    _, raw = U.simulate_XLFM_image(OTF, vol, seed=SEED, **kw)
    assert np.array_equal(bits(host(raw)), bits(host(ops.rand_poisson(clean[0].contiguous(), SEED, n_samples=1))))
    hn = host(noisy)
    assert np.array_equal(hn, np.rint(hn)) and hn.min() >= 0
