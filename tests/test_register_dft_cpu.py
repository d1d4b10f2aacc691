"""CPU: the up-sampled-DFT refinement of rigid frame registration without a GPU -- the numpy restatement
tests/register_dft_ref.py against the definition evaluated with numpy.exp, its root tables against long double, u = 1 against
numpy.fft.irfft2, exact recovery of a planted band-limited displacement, what the refinement is for (a smaller error than the
three-point parabola on the planted scene), the guards of the fine peak, the argument checks of the new entry points through the
built library and the refusals the Python layer decides before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import register_dft_ref as D
import register_ref as R

EPS = 2.0 ** -53                                                         # the unit roundoff of float64


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


def unit_spectra(N, H, W, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((N, H, W // 2 + 1)) + 1j * rng.standard_normal((N, H, W // 2 + 1))
    return (z / np.abs(z)).astype(np.complex64)                            # moduli 1, as whitening leaves them


def term_bound(Rw, H, W, terms):
    """terms * 2^-53 * (the sum of the moduli of the terms of a map): a sum of n terms in any order is off by at most
    (n - 1) eps times the sum of their moduli, and every term -- two twiddles of a few ulp each, four products, a difference --
    carries less than 40 eps of its own modulus."""
    return terms * EPS * float(2.0 * np.abs(Rw.astype(np.complex128)).sum(axis=(1, 2)).max()) / (H * W)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("H,W", [(8, 9), (9, 8), (37, 45)])
@pytest.mark.parametrize("u", [1, 2, 16])
def test_restatement_against_the_definition(H, W, u):
    """Both sides sum the same H K terms of modulus <= 2 |R| / (H W).  The restatement adds K terms in a row, ceil(H / 8) rows in a
    segment and 8 segments (K + ceil(H / 8) + 8 additions on any path), numpy.einsum adds H K terms in an order of its own, and a
    term's own error is below 40 eps on either side: the difference is at most (K + ceil(H / 8) + 8 + H K + 80) eps sum |terms|."""
    K = W // 2 + 1
    Rw = unit_spectra(2, H, W, 10 * H + W)
    for r in sorted({1, u}):
        for ip in ([[2, -3], [-1, 1]], [[0, 0], [-3, H + 2]]):           # positive, negative and beyond-the-frame peaks
            got, want = D.upsample(Rw, np.array(ip), (H, W), u, r), D.brute(Rw, np.array(ip), (H, W), u, r)
            bound = term_bound(Rw, H, W, K + (H + 7) // 8 + 8 + H * K + 80)
            diff = float(np.abs(got - want).max())
            print(f"{H} x {W}, u {u}, r {r}: |restatement - definition| = {diff:.3e}, bound {bound:.3e}")
            assert got.shape == (2, 2 * r + 1, 2 * r + 1) and diff <= bound


@pytest.mark.parametrize("M", [1, 2, 7, 8, 18, 37 * 16, 45 * 16, 96 * 16])
def test_root_table_against_long_double(M):
    """The angle is pi p / q with p / q <= 1 / 4 exact.  fl(pi) is off by 0.35 eps of pi, the product and the quotient round once
    each: the float64 angle is off by at most 2.35 eps of itself.  sin has condition t / tan t <= 1 and cos t tan t <= pi / 4 on
    [0, pi / 4], so the argument costs at most 2.35 eps of the value, which is at most 2.35 ulp; the library's cos and sin are
    within 1 ulp.  Bound: 3.35 ulp, asserted as 3.5 (the long double reference has 11 more bits)."""
    assert np.finfo(np.longdouble).nmant >= 63
    tab = D.roots(M)
    pi = 4 * np.arctan(np.longdouble(1))
    worst = 0.0
    for k in range(M):
        p, q, swap, sc, ss = D.reduce_octant(k, M)
        assert 0 <= 4 * p <= q
        t = pi * np.longdouble(p) / np.longdouble(q)
        c, s = (np.sin(t), np.cos(t)) if swap else (np.cos(t), np.sin(t))
        for got, want in ((tab[k, 0], sc * c), (tab[k, 1], ss * s)):
            err = abs(np.longdouble(got) - want)
            if err:
                worst = max(worst, float(err / np.spacing(abs(got)) if got else np.inf))
    print(f"M = {M}: worst root error {worst:.3f} ulp (bound 3.5)")
    assert worst <= 3.5
    assert tuple(tab[0]) == (1.0, 0.0)
    if M % 4 == 0:
        assert tuple(tab[M // 4]) == (0.0, 1.0) and tuple(tab[M // 2]) == (-1.0, 0.0) and tuple(tab[3 * M // 4]) == (0.0, -1.0)


def test_python_root_table_is_the_restatement():
    from cwfa_amd import ops
    for M in (1, 5, 16, 45 * 16):
        got = ops.reg_roots(M)
        assert got.dtype == torch.float64 and tuple(got.shape) == (M, 2)
        assert np.array_equal(got.numpy().view(np.uint64), D.roots(M).view(np.uint64))


@pytest.mark.parametrize("H,W", [(8, 9), (9, 8), (37, 45), (64, 96)])
def test_factor_one_is_the_inverse_transform(H, W):
    """u = 1, r = 1: the nine points are the map's own samples.  pocketfft's error is below that of H K terms added in any order,
    the restatement's as in the test above: the same bound."""
    K = W // 2 + 1
    Rw = unit_spectra(3, H, W, H + W)
    ip = np.array([[0, 0], [3, -2], [-H // 2, W - 1]])
    got = D.upsample(Rw, ip, (H, W), 1, 1)
    c = np.fft.irfft2(Rw.astype(np.complex128), s=(H, W))
    bound = term_bound(Rw, H, W, K + (H + 7) // 8 + 8 + H * K + 80)
    worst = 0.0
    for n in range(3):
        for jy in (-1, 0, 1):
            for jx in (-1, 0, 1):
                worst = max(worst, abs(got[n, jy + 1, jx + 1] - c[n, (ip[n, 0] + jy) % H, (ip[n, 1] + jx) % W]))
    print(f"{H} x {W}: |C - irfft2| = {worst:.3e}, bound {bound:.3e}, map maximum {np.abs(c).max():.3f}")
    assert worst <= bound


# ------------------------------------------------------------------------------------------------ exactness
def moved(t, d):
    """The template moved circularly by d = (dy, dx) with a Fourier phase ramp (frame[p] = t[p - d]), in float64, as fp32."""
    H, W = t.shape
    ky, kx = np.fft.fftfreq(H)[:, None], np.fft.rfftfreq(W)[None, :]
    return np.fft.irfft2(np.fft.rfft2(t.astype(np.float64)) * np.exp(-2j * np.pi * (ky * d[0] + kx * d[1])), s=(H, W)).astype(np.float32)


def exactness(H, W, seed=3, draws=20):
    rng = np.random.default_rng(seed)
    t = rng.random((H, W)).astype(np.float32)
    d = rng.integers(-32, 33, size=(draws, 2)) / 16.0                       # multiples of 1/16 px, |d| <= 2
    frames = np.stack([moved(t, d[n]) for n in range(draws)])
    s, pk, ip, C = D.estimate_shifts(frames, t, 3, 0, 0.0, u=16)
    U = C.shape[1]
    hits = 0
    for n in range(draws):
        jy, jx = divmod(int(np.argmax(C[n])), U)
        hits += (ip[n, 0] * 16 + jy - 16, ip[n, 1] * 16 + jx - 16) == (round(d[n, 0] * 16), round(d[n, 1] * 16))
    return hits, draws, float(np.abs(s.astype(np.float64) - d).max())


# MEASURED on the restatement at 37 x 45 (20 draws): 20 of 20 fine maxima on the planted grid point, the vertex at most 2.494e-09 px
# off it; the bound is 4 times that.  (64 x 96, where the Nyquist rule enters: 20 of 20 hits, at most 1.346e-02 px off -- reported.)
EXACT_OFFSET_MEASURED = 2.494e-09
EXACT_OFFSET_BOUND = 4 * EXACT_OFFSET_MEASURED


def test_a_planted_band_limited_displacement_is_recovered_exactly():
    hits, draws, off = exactness(37, 45)
    print(f"37 x 45: {hits} of {draws} fine maxima on the planted grid point, vertex offset {off:.3e} px (measured {EXACT_OFFSET_MEASURED:.3e})")
    assert hits == draws and off <= EXACT_OFFSET_BOUND
    hits, draws, off = exactness(64, 96)
    print(f"64 x 96 (reported, not asserted): {hits} of {draws} hits, vertex offset {off:.3e} px")


# ------------------------------------------------------------------------------------------------ purpose
# MEASURED (restatement, seeds 0 .. 7, max_shift 6, taper 4, smooth 0, u 16, the 7 moved frames x 2 axes x 8 seeds = 112 components),
# median / 90th percentile / worst error in px, and the components where "dft" is closer:
#   37 x 45    parabola 0.0786 / 0.1814 / 0.2886    dft 0.0420 / 0.1308 / 0.2096    79 of 112
#   64 x 96    parabola 0.0633 / 0.1238 / 0.1791    dft 0.0203 / 0.0547 / 0.0953    95 of 112
# Not asserted: smooth 0.75: 37 x 45 0.1080 / 0.2472 / 0.3851 against 0.0889 / 0.2059 / 0.3129 (69 of 112), 64 x 96 0.0412 / 0.0987 /
# 0.2314 against 0.0303 / 0.0744 / 0.1560 (68 of 112); 128 x 160 with 365 blobs, smooth 0: 0.0538 / 0.1064 / 0.1264 against 0.0127 /
# 0.0278 / 0.0447 (93 of 112).
@pytest.mark.parametrize("H,W", [(37, 45), (64, 96)])
def test_dft_refinement_beats_the_parabola_on_the_planted_scene(H, W):
    tabs = (D.roots(W * 16), D.roots(H * 16))
    ep, ed = [], []
    for seed in range(8):
        sc = R.scene(seed, H, W, subpixel=True)
        s0, _, _ = R.peak(R.correlate(sc.frames, sc.template, taper=4), 6)
        s1, pk, ip, _ = D.estimate_shifts(sc.frames, sc.template, 6, 4, 0.0, u=16, tables=tabs)
        assert np.all(np.abs(ip - sc.shifts) < 1.0) and np.isfinite(pk).all()
        ep.append(np.abs(s0 - sc.shifts)[1:])
        ed.append(np.abs(s1 - sc.shifts)[1:])
    ep, ed = np.concatenate(ep).ravel(), np.concatenate(ed).ravel()
    print(f"{H} x {W}: parabola median {np.median(ep):.4f} worst {ep.max():.4f}; dft median {np.median(ed):.4f} worst {ed.max():.4f}; "
          f"closer in {int((ed < ep).sum())} of {ed.size}")
    assert ed.max() < ep.max() and np.median(ed) < np.median(ep)


# ------------------------------------------------------------------------------------------------ the fine peak's guards
def test_fine_peak_guards():
    u, U = 4, 9
    yy, xx = np.mgrid[0:U, 0:U].astype(np.float64)
    bowl = lambda cy, cx: 1.0 - 0.01 * ((yy - cy) ** 2 + (xx - cx) ** 2)
    C = np.stack([bowl(4.25, 3.0), bowl(-2.0, 8.6), np.full((U, U), np.nan), np.full((U, U), 0.5), bowl(4.0, 4.0), np.full((U, U), np.nan)])
    C[3, 2, 7] = C[3, 6, 1] = 0.75                                          # a tie: the lower row-major index
    C[4, 0, 0], C[4, 8, 8], C[4, 4, 5] = np.inf, -np.inf, np.nan            # inf is a maximum like any other; it sits in a corner
    C[5, 3, 3] = -np.inf                                                    # nothing finite
    ip = np.array([[2, -3], [0, 5], [1, 1], [-1, 0], [0, 0], [4, -4]], dtype=np.int32)
    s, pk = D.fine_peak(C, ip, u)
    assert np.allclose(s[0], [2 + 0.25 / u, -3 - 1.0 / u], atol=1e-6) and pk[0] == np.float32(C[0, 4, 3]), "a parabola is fitted exactly"
    assert s[1, 0] == np.float32(0 - 4 / u) and abs(s[1, 1] - (5 + 4 / u)) < 1e-6, "the maximum on the border: no vertex on that axis"
    assert tuple(s[1]) == (-1.0, 6.0), "both axes on the border here: (0, 8)"
    assert tuple(s[2]) == (1.0, 1.0) and np.isnan(pk[2]), "no finite value: the integer peak, peak NaN"
    assert tuple(s[3]) == (np.float32(-1 + (2 - 4) / u), np.float32((7 - 4) / u)) and pk[3] == 0.75, "ties go to the lowest index"
    assert tuple(s[4]) == (-1.0, -1.0) and pk[4] == np.inf
    assert tuple(s[5]) == (4.0, -4.0) and np.isnan(pk[5])
    # the integer stage's NaN peak: the frame is kept as it is and its map is not read
    s0, p0 = np.float32([[0, 0]] * 6), np.float32([1, np.nan, 1, 1, 1, 1])
    s2, p2 = D.fine_peak(C, ip, u, s0, p0)
    assert tuple(s2[1]) == (0.0, 0.0) and np.isnan(p2[1]) and np.array_equal(np.delete(s2, 1, 0), np.delete(s, 1, 0))
    # -0 and +0 are one value; NaN is below everything, -inf included
    Z = np.full((1, 3, 3), -0.0)
    Z[0, 1, 1] = 0.0
    assert tuple(D.fine_peak(Z, ip[:1], 1)[0][0]) == (1.0, -4.0), "the first -0 wins the tie with +0"
    Z = np.full((1, 3, 3), np.nan)
    Z[0, 2, 1] = -np.inf
    Z[0, 2, 2] = -1e300
    s, pk = D.fine_peak(Z, ip[:1], 2)
    assert tuple(s[0]) == (2.5, -2.5) and pk[0] == -np.inf, "(float)-1e300 overflows to -inf; NaN neighbours give no vertex"


# ------------------------------------------------------------------------------------------------ the entry points' arguments
def test_reg_upsample_arguments(L, ptr):
    R_, ipk, rx, ry, C, ws = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(6))

    def call(R=R_, N=2, H=5, W=8, fs=25, ipeak=ipk, u=4, r=4, rootx=rx, rooty=ry, C=C, ws=ws):
        return L.cwfa_reg_upsample_c64(R, N, H, W, fs, ipeak, u, r, rootx, rooty, C, ws, None)

    for k in ("R", "ipeak", "rootx", "rooty", "C", "ws"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_upsample_c64: null" in L.cwfa_last_error(), k
    assert call(N=-1) == -2 and b"negative" in L.cwfa_last_error()
    assert call(H=0) == -2 and call(W=0) == -2 and call(H=-5) == -2 and b"a frame of" in L.cwfa_last_error()
    assert call(u=0) == -1 and call(r=0) == -1 and call(u=-1) == -1 and b"at least 1" in L.cwfa_last_error()
    assert call(fs=24) == -1 and call(fs=-25) == -1 and b"stride" in L.cwfa_last_error()
    assert call(H=1 << 16, W=1 << 15, fs=1 << 40) == -2 and call(u=1 << 29) == -2 and call(r=1 << 14) == -2 and b"too large" in L.cwfa_last_error()
    for k in ("R", "ipeak", "C"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 4)}) == -3 and b"8-byte" in L.cwfa_last_error(), k
    for k in ("rootx", "rooty", "ws"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 8)}) == -3 and b"16-byte" in L.cwfa_last_error(), k
    assert call(N=0) == 0, "empty: no launch"
    assert L.cwfa_set_option(b"reg_upsample_stages", 8) == -1 and L.cwfa_set_option(b"reg_upsample_stages", -1) == -1
    assert b"reg_upsample_stages" in L.cwfa_last_error() and L.cwfa_set_option(b"reg_upsample_stages", 7) == 0
    wb = L.cwfa_reg_upsample_workspace_bytes
    assert wb(2, 5, 8, 4) == 2 * 9 * (5 + 2 * 5) * 16 and wb(0, 5, 8, 4) == 0 and wb(1, 1, 1, 1) == 3 * 3 * 16
    assert wb(16, 2160, 2160, 16) == 16 * 33 * (1081 + 4320) * 16
    assert wb(-1, 5, 8, 4) == -1 and wb(1, 0, 8, 4) == -1 and wb(1, 5, 0, 4) == -1 and wb(1, 5, 8, 0) == -1 and wb(1, 5, 8, 1 << 14) == -1


def test_reg_fine_peak_arguments(L, ptr):
    C, ipk, shifts, peak = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(4))

    def call(C=C, ipeak=ipk, N=2, U=9, u=4, keep=0, shifts=shifts, peak=peak):
        return L.cwfa_reg_fine_peak_f64(C, ipeak, N, U, u, keep, shifts, peak, None)

    for k in ("C", "ipeak", "shifts", "peak"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_fine_peak_f64: null" in L.cwfa_last_error(), k
    assert call(keep=2) == -1 and call(keep=-1) == -1 and b"keep" in L.cwfa_last_error()
    assert call(N=-1) == -2 and b"negative" in L.cwfa_last_error()
    assert call(u=0) == -1 and b"at least 1" in L.cwfa_last_error()
    assert call(U=1) == -2 and call(U=8) == -2 and call(U=-3) == -2 and call(U=(1 << 15) + 1) == -2 and b"2 r + 1" in L.cwfa_last_error()
    for k in ("C", "ipeak", "shifts"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 4)}) == -3 and b"8-byte" in L.cwfa_last_error(), k
    assert call(peak=ctypes.c_void_p(ptr.value + 2)) == -3
    assert call(N=0) == 0, "empty: no launch"


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_python_layer_refuses_before_any_device_work():
    from cwfa_amd import ops
    from cwfa_amd.XLFMDataset import estimate_shifts, register_frames
    Rw = torch.zeros(4, 40, 25, dtype=torch.complex64)
    ip = torch.zeros(4, 2, dtype=torch.int32)
    for bad in (0, -1, 2.0, 1.5, "4", None, True):
        with pytest.raises(ValueError, match="upsample"):
            ops.reg_upsample(Rw, ip, (40, 48), bad)
        with pytest.raises(ValueError, match="upsample"):
            ops.reg_fine_peak(torch.zeros(4, 9, 9, dtype=torch.float64), ip, bad)
    for bad in (0, -2, 2.0, "1"):
        with pytest.raises(ValueError, match="radius"):
            ops.reg_upsample(Rw, ip, (40, 48), 4, radius=bad)
    with pytest.raises(TypeError, match="complex64"):
        ops.reg_upsample(Rw.to(torch.complex128), ip, (40, 48), 4)
    with pytest.raises(TypeError, match="complex64"):
        ops.reg_upsample(torch.zeros(4, 40, 25), ip, (40, 48), 4)
    for shape in ((40, 50), (41, 48), (40, 24)):
        with pytest.raises(ValueError, match="spectra of"):
            ops.reg_upsample(Rw, ip, shape, 4)
    with pytest.raises(ValueError, match="spectra of"):
        ops.reg_upsample(Rw[0], ip, (40, 48), 4)
    with pytest.raises(ValueError, match="shape"):
        ops.reg_upsample(Rw, ip, (40, 48, 1), 4)
    for bad in (ip[:3], ip.long(), ip.float(), ip.t(), None):
        with pytest.raises(ValueError, match="ipeak"):
            ops.reg_upsample(Rw, bad, (40, 48), 4)
        with pytest.raises(ValueError, match="ipeak"):
            ops.reg_fine_peak(torch.zeros(4, 9, 9, dtype=torch.float64), bad, 4)
    with pytest.raises(TypeError, match="float64"):
        ops.reg_fine_peak(torch.zeros(4, 9, 9), ip, 4)
    for bad in (torch.zeros(4, 9, 8, dtype=torch.float64), torch.zeros(4, 8, 8, dtype=torch.float64), torch.zeros(4, 1, 1, dtype=torch.float64),
                torch.zeros(9, 9, dtype=torch.float64)):
        with pytest.raises(ValueError, match="2 r \\+ 1"):
            ops.reg_fine_peak(bad, ip, 4)
    for call in (lambda: ops.reg_upsample(Rw, ip, (40, 48), 4), lambda: ops.reg_upsample(Rw, ip, (40, 49), 16, radius=3),
                 lambda: ops.reg_fine_peak(torch.zeros(4, 9, 9, dtype=torch.float64), ip, 4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    s, t = torch.zeros(4, 40, 48), torch.zeros(40, 48)
    for fn in (estimate_shifts, register_frames):
        with pytest.raises(ValueError, match="subpixel"):
            fn(s, t, subpixel="fft")
        for bad in (0, 2.5, None):
            with pytest.raises(ValueError, match="upsample"):
                fn(s, t, subpixel="dft", upsample=bad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(s, t, subpixel="dft", upsample=4)


def test_the_new_keyword_is_last():
    import inspect
    from cwfa_amd.XLFMDataset import estimate_shifts, register_frames
    for fn, before in ((estimate_shifts, "chunk"), (register_frames, "out")):
        names = list(inspect.signature(fn).parameters)
        assert names[-1] == "upsample" and names[-2] == before and inspect.signature(fn).parameters["upsample"].default == 16
