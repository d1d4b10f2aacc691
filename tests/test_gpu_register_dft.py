"""GPU: the up-sampled-DFT refinement of rigid frame registration.  ``ops.reg_upsample`` and
``ops.reg_fine_peak`` bit for bit against the numpy restatement tests/register_dft_ref.py on handed-in spectra, peaks and maps (no
FFT difference enters); whether ``irfft2`` leaves the spectra it reads alone, which ``estimate_shifts`` relies on; then
``estimate_shifts(subpixel="dft")`` end to end against the restatement on the exactness scene and on the planted scene, where the
device's own output has to beat the device's parabola; and the two older sub-pixel modes, whose bits the new path must not touch."""
import functools

import numpy as np
import pytest
import torch

import register_dft_ref as D
import register_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 7), (2, 37, 45), (8, 64, 96)]                 # odd and even sizes; 37 and 5 rows are no multiple of a workgroup's
PEAKS = [(0, 0), (6, -6), (-6, 6), (-1, 3), (101, -77), (3, 0), (-2, -5), (0, 1)]   # 0, +-max_shift, the wrap side, beyond the frame


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def tables(H, W, u):
    return D.roots(W * u), D.roots(H * u)


@functools.lru_cache(maxsize=None)
def case(N, H, W):
    """Spectra of modulus 1 (as whitening leaves them) with a zero bin, and integer peaks."""
    rng = np.random.default_rng(5 + 100 * N + 10 * H + W)
    K = W // 2 + 1
    z = rng.standard_normal((N, H, K)) + 1j * rng.standard_normal((N, H, K))
    Rw = (z / np.abs(z)).astype(np.complex64)
    Rw[0, 0, 0] = 0
    Rw[N - 1, H - 1, K - 1] = 0
    return Rw, np.array([PEAKS[n % len(PEAKS)] for n in range(N)], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def reference(N, H, W, u, r):
    Rw, ip = case(N, H, W)
    return D.upsample(Rw, ip, (H, W), u, r, tables(H, W, u))


@pytest.fixture(scope="module", autouse=True)
def parabola_before(request):
    """The two older modes on the planted scene BEFORE anything of this module has run: the root-table cache is empty, so no
    up-sampled DFT has run in the process."""
    from cwfa_amd import ops
    from cwfa_amd.XLFMDataset import estimate_shifts
    fresh = not ops._REG_ROOTS
    sc = R.scene(0, 37, 45, subpixel=True)
    f, t = torch.from_numpy(sc.frames).cuda(), torch.from_numpy(sc.template).cuda()
    out = {sub: tuple(a.cpu().numpy() for a in estimate_shifts(f, t, max_shift=6, taper=4, subpixel=sub)) for sub in (True, False)}
    return fresh, out


# ------------------------------------------------------------------------------------------------ the up-sampled DFT
@pytest.mark.parametrize("u", [1, 2, 16])
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_upsample_bit_for_bit(N, H, W, u):
    from cwfa_amd import ops
    Rw, ip = case(N, H, W)
    Rd, ipd = torch.from_numpy(Rw).cuda(), torch.from_numpy(ip).cuda()
    for r in sorted({1, u}):
        want = reference(N, H, W, u, r)
        assert np.isfinite(want).all()
        got = ops.reg_upsample(Rd, ipd, (H, W), u, radius=r)
        assert got.dtype == torch.float64 and tuple(got.shape) == (N, 2 * r + 1, 2 * r + 1) and same_bits(got, want), (u, r)
        out = torch.empty_like(got)
        assert ops.reg_upsample(Rd, ipd, (H, W), u, radius=r, out=out) is out and same_bits(out, want), "two runs are equal"
    assert same_bits(ops.reg_upsample(Rd, ipd, (H, W), u), reference(N, H, W, u, u)), "the default radius is the factor: +-1 px"
    assert same_bits(Rd, Rw), "the spectra are read only"


@pytest.mark.parametrize("N,H,W", SHAPES[1:])
def test_upsample_with_a_frame_stride(N, H, W):
    from cwfa_amd import ops
    Rw, ip = case(N, H, W)
    K, pad = W // 2 + 1, 3
    buf = torch.full((N, H * K + pad), complex(3e4, -3e4), dtype=torch.complex64, device="cuda")   # the gaps hold what nothing may read
    view = buf[:, :H * K].view(N, H, K)
    view.copy_(torch.from_numpy(Rw))
    assert view.stride(0) == H * K + pad and view.data_ptr() == buf.data_ptr()
    assert same_bits(ops.reg_upsample(view, torch.from_numpy(ip).cuda(), (H, W), 2), reference(N, H, W, 2, 2))
    tail = ops.reg_upsample(view[1:], torch.from_numpy(ip[1:]).cuda(), (H, W), 2)                    # a base off the buffer's start
    assert same_bits(tail, reference(N, H, W, 2, 2)[1:])


def test_a_nan_bin_stays_in_its_frame():
    from cwfa_amd import ops
    N, H, W, u = 3, 5, 7, 2
    Rw, ip = (a.copy() for a in case(N, H, W))
    Rw[1, 2, 1] = complex(np.nan, 0.0)
    got = ops.reg_upsample(torch.from_numpy(Rw).cuda(), torch.from_numpy(ip).cuda(), (H, W), u).cpu().numpy()
    want = reference(N, H, W, u, u)
    assert np.isnan(got[1]).all() and same_bits(got[0], want[0]) and same_bits(got[2], want[2])
    s, pk = ops.reg_fine_peak(torch.from_numpy(got).cuda(), torch.from_numpy(ip).cuda(), u)
    ws, wpk = D.fine_peak(got, ip, u)
    assert same_bits(s, ws) and np.isnan(pk[1].item()) and tuple(s[1].tolist()) == tuple(float(v) for v in ip[1]), "the integer peak, peak NaN"
    assert same_bits(pk[[0, 2]], wpk[[0, 2]])


def test_no_frames_launch_nothing():
    from cwfa_amd import ops
    got = ops.reg_upsample(torch.zeros(0, 5, 4, dtype=torch.complex64, device="cuda"), torch.zeros(0, 2, dtype=torch.int32, device="cuda"), (5, 7), 4)
    assert tuple(got.shape) == (0, 9, 9)
    s, pk = ops.reg_fine_peak(got, torch.zeros(0, 2, dtype=torch.int32, device="cuda"), 4)
    assert tuple(s.shape) == (0, 2) and tuple(pk.shape) == (0,)
    torch.cuda.synchronize()


def test_the_workspace_is_exactly_as_long_as_reported():
    from cwfa_amd import _lib, ops
    N, H, W, u = 2, 37, 45, 2
    Rw, ip = case(N, H, W)
    nbytes = int(_lib.lib().cwfa_reg_upsample_workspace_bytes(N, H, W, u))
    assert nbytes == 16 * N * 5 * (23 + 2 * 37) and nbytes % 8 == 0
    guard = 4096
    buf = torch.full((nbytes // 8 + guard,), -7.25, dtype=torch.float64, device="cuda")
    got = ops.reg_upsample(torch.from_numpy(Rw).cuda(), torch.from_numpy(ip).cuda(), (H, W), u, workspace=buf[:nbytes // 8])
    assert same_bits(got, reference(N, H, W, u, u))
    assert bool((buf[nbytes // 8:] == -7.25).all()), "nothing is written behind the workspace"
    assert not bool((buf[:nbytes // 8] == -7.25).any()), "and all of it is used"
    with pytest.raises(ValueError, match="workspace"):
        ops.reg_upsample(torch.from_numpy(Rw).cuda(), torch.from_numpy(ip).cuda(), (H, W), u, workspace=buf[:nbytes // 8 - 1])


# ------------------------------------------------------------------------------------------------ the fine peak
def test_fine_peak_bit_for_bit():
    from cwfa_amd import ops
    rng = np.random.default_rng(11)
    for U, u in ((3, 1), (9, 4), (33, 16), (41, 16)):                      # 33 x 33 and 41 x 41: more cells than a workgroup has threads
        N = 12
        C = 0.05 * rng.standard_normal((N, U, U))
        yy, xx = np.mgrid[0:U, 0:U].astype(np.float64)
        for n in range(6):                                                  # a smooth peak somewhere, one on every border
            cy, cx = ((U - 1) * rng.random(), (U - 1) * rng.random()) if n < 2 else [(0, U / 2), (U - 1, 1.3), (U / 3, 0), (1.2, U - 1)][n - 2]
            C[n] += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * (U / 4) ** 2))
        C[6] = 0.25                                                         # a plateau: the lowest index, den = 0
        C[7, :, :] = 0.5
        C[7, 1, U - 2] = C[7, U - 2, 1] = 0.75                              # a tie
        C[8, 0, 1], C[8, U - 1, U - 1], C[8, 1, 1] = np.nan, -np.inf, np.inf
        C[9] = -0.0
        C[9, U // 2, U // 2] = 0.0
        C[10] = np.nan                                                      # nothing finite
        C[11] = np.nan
        C[11, 1, 1], C[11, 1, 2] = -np.inf, -1e300                          # one finite value among NaN; (float) of it is -inf
        ip = rng.integers(-9, 10, size=(N, 2)).astype(np.int32)
        Cd, ipd = torch.from_numpy(C).cuda(), torch.from_numpy(ip).cuda()
        ws, wpk = D.fine_peak(C, ip, u)
        s, pk = ops.reg_fine_peak(Cd, ipd, u)
        assert s.dtype == torch.float32 and same_bits(s, ws), (U, u)
        assert np.array_equal(np.isnan(wpk), np.isnan(pk.cpu().numpy())) and same_bits(pk.nan_to_num(7.0), np.nan_to_num(wpk, nan=7.0))
        assert np.isnan(wpk[10]) and tuple(ws[10]) == tuple(np.float32(ip[10])) and wpk[8] == np.inf and wpk[11] == -np.inf
        s2, pk2 = ops.reg_fine_peak(Cd, ipd, u)
        assert same_bits(s2, s) and same_bits(pk2.nan_to_num(7.0), pk.nan_to_num(7.0)), "two runs are equal"
        # the integer stage's results handed in: the frame whose integer peak was NaN is kept, every other frame is as above
        s0 = torch.from_numpy(ip.astype(np.float32)).cuda()
        p0 = torch.ones(N, device="cuda")
        s0[3], p0[3] = 0.0, float("nan")
        out = ops.reg_fine_peak(Cd, ipd, u, out=(s0, p0))
        assert out[0] is s0 and out[1] is p0
        w2, wp2 = D.fine_peak(C, ip, u, np.where(np.arange(N)[:, None] == 3, 0.0, ip).astype(np.float32), np.where(np.arange(N) == 3, np.nan, 1.0))
        assert same_bits(s0, w2) and tuple(s0[3].tolist()) == (0.0, 0.0) and np.isnan(p0[3].item())
        assert same_bits(p0.nan_to_num(7.0), np.nan_to_num(wp2, nan=7.0))


# ------------------------------------------------------------------------------------------------ the transform's input
@pytest.mark.parametrize("N,H,W", [(8, 37, 45), (8, 64, 96), (16, 128, 160)])
def test_irfft2_leaves_its_input_alone(N, H, W):
    """``estimate_shifts`` reads the whitened spectra again after ``torch.fft.irfft2`` has transformed them."""
    g = torch.Generator(device="cuda").manual_seed(H)
    F = torch.fft.rfft2(torch.randn(N, H, W, device="cuda", generator=g)).contiguous()
    before = F.clone()
    c = torch.fft.irfft2(F, s=(H, W))
    torch.cuda.synchronize()
    assert tuple(c.shape) == (N, H, W) and same_bits(torch.view_as_real(F), torch.view_as_real(before))


# ------------------------------------------------------------------------------------------------ end to end
def moved(t, d):
    H, W = t.shape
    ky, kx = np.fft.fftfreq(H)[:, None], np.fft.rfftfreq(W)[None, :]
    return np.fft.irfft2(np.fft.rfft2(t.astype(np.float64)) * np.exp(-2j * np.pi * (ky * d[0] + kx * d[1])), s=(H, W)).astype(np.float32)


# The largest |device - restatement| of the "dft" shifts, observed on the MI355X.  The two differ only in the transforms (rocFFT in
# fp32 against numpy.fft in float64): the fine map moves by the transforms' rounding, a fine maximum may move to the neighbouring grid
# point, and the parabola on the fine grid keeps the shift continuous across that.  The bounds are 4 x the observations.
OBSERVED_EXACT_DIFF = 1.490e-08    # px, the exactness scene (37 x 45, 20 draws); also the device's distance from the planted values
OBSERVED_SCENE_DIFF = 1.621e-06    # px, the planted scene, seeds 0 .. 7: 1.621e-06 at 37 x 45, 2.980e-07 at 64 x 96


def test_exactness_scene_on_the_device():
    from cwfa_amd.XLFMDataset import estimate_shifts
    rng = np.random.default_rng(3)
    t = rng.random((37, 45)).astype(np.float32)
    d = rng.integers(-32, 33, size=(20, 2)) / 16.0
    frames = np.stack([moved(t, d[n]) for n in range(20)])
    want, wpk, _, _ = D.estimate_shifts(frames, t, 3, 0, 0.0, u=16)
    got, pk = estimate_shifts(torch.from_numpy(frames).cuda(), torch.from_numpy(t).cuda(), max_shift=3, taper=0, subpixel="dft", upsample=16)
    got = got.cpu().numpy()
    diff, off = float(np.abs(got - want).max()), float(np.abs(got.astype(np.float64) - d).max())
    print(f"exactness scene: |device - restatement| = {diff:.3e} px, |device - planted| = {off:.3e} px")
    assert diff <= 4 * OBSERVED_EXACT_DIFF and float(np.abs(pk.cpu().numpy() - wpk).max()) < 1e-3


@pytest.mark.parametrize("H,W", [(37, 45), (64, 96)])
def test_planted_scene_on_the_device(H, W):
    from cwfa_amd.XLFMDataset import estimate_shifts, register_frames
    tabs = tables(H, W, 16)
    worst, worst3, ep, ed = 0.0, 0.0, [], []
    for seed in range(8):
        sc = R.scene(seed, H, W, subpixel=True)
        f, t = torch.from_numpy(sc.frames).cuda(), torch.from_numpy(sc.template).cuda()
        want, wpk, _, _ = D.estimate_shifts(sc.frames, sc.template, 6, 4, 0.0, u=16, tables=tabs)
        got, pk = estimate_shifts(f, t, max_shift=6, taper=4, subpixel="dft", upsample=16)
        par, _ = estimate_shifts(f, t, max_shift=6, taper=4, subpixel=True)
        got, par = got.cpu().numpy(), par.cpu().numpy()
        worst = max(worst, float(np.abs(got - want).max()))
        assert float(np.abs(pk.cpu().numpy() - wpk).max()) < 1e-3
        ep.append(np.abs(par - sc.shifts)[1:])
        ed.append(np.abs(got - sc.shifts)[1:])
        if seed == 0:
            got3, pk3 = estimate_shifts(f, t, max_shift=6, taper=4, subpixel="dft", upsample=16, chunk=3)     # slices of the outputs
            reg = register_frames(f, t, max_shift=6, taper=4, subpixel="dft", upsample=16, chunk=3)
            assert same_bits(reg.shifts, got3) and same_bits(reg.peak, pk3), "register_frames passes it through"
            assert same_bits(reg.frames, R.shift(sc.frames, got3.cpu().numpy()))
            worst3 = float(np.abs(got3.cpu().numpy() - want).max())
    ep, ed = np.concatenate(ep).ravel(), np.concatenate(ed).ravel()
    print(f"{H} x {W}: |device - restatement| = {worst:.3e} px ({worst3:.3e} in chunks of 3, seed 0); device parabola median {np.median(ep):.4f} worst {ep.max():.4f}, "
          f"device dft median {np.median(ed):.4f} worst {ed.max():.4f}")
    assert max(worst, worst3) <= 4 * OBSERVED_SCENE_DIFF
    assert ed.max() < ep.max() and np.median(ed) < np.median(ep), "what the refinement is for, on the device's own output"


def test_the_older_modes_keep_their_bits(parabola_before):
    from cwfa_amd import ops
    from cwfa_amd.XLFMDataset import estimate_shifts
    fresh, before = parabola_before
    assert fresh, "the module fixture ran after an up-sampled DFT"
    sc = R.scene(0, 37, 45, subpixel=True)
    f, t = torch.from_numpy(sc.frames).cuda(), torch.from_numpy(sc.template).cuda()
    estimate_shifts(f, t, max_shift=6, taper=4, subpixel="dft")
    assert ops._REG_ROOTS, "the new path has run"
    for sub in (True, False):
        s, pk = estimate_shifts(f, t, max_shift=6, taper=4, subpixel=sub)
        assert same_bits(s, before[sub][0]) and same_bits(pk, before[sub][1]), sub
        want, _, wpk = R.peak(R.correlate(sc.frames, sc.template, 4), 6, sub)
        assert float(np.abs(s.cpu().numpy() - want).max()) <= 4 * 4.768e-07
