"""CPU: rigid frame registration without a GPU -- the numpy restatement tests/register_ref.py checked against
itself (sign convention, ties, NaN, the parabola's guards, zero-weight taps, nearest), planted integer and sub-pixel displacements
on the scene, the argument validation of the four entry points through the built library, and the refusals the Python layer
decides before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import register_ref as R

SIZES = ((37, 45), (64, 96))
SEEDS = tuple(range(8))
# The worst |estimate - planted| of the restatement over SIZES x SEEDS on the sub-pixel scene (30 blobs of sigma 1 - 1.8 px,
# intermittent activity, 2 % noise, taper 4, max_shift 6, the still stack's lower median as template), in pixels: MEASURED 0.2886
# (37 x 45, seed 5); per size 0.289 and 0.179.  A three-point parabola through a phase-correlation peak is biased toward the
# integer: the peak of a whitened correlation is far narrower than a parabola.  Recorded, not tuned.  What is asserted is what the
# estimator is for: the integer peak is the planted displacement's floor or ceiling, and the refined estimate is no further off
# than 0.5 px, the worst case of rounding to the nearest integer -- a refinement that does worse than none would be a defect.
SUBPIXEL_WORST_MEASURED = 0.2886
SUBPIXEL_BOUND = 0.5


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


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("d", [(0, 0), (3, -2), (-4, 1), (-1, -5)])
def test_sign_convention_template_displaced_by_d_reports_d(d):
    rng = np.random.default_rng(7)
    t = rng.random((24, 30)).astype(np.float32)
    frame = np.roll(t, d, axis=(0, 1))                                     # frame[p] = t[p - d], cyclic: the peak is 1 up to rounding
    s, ip, pk = R.peak(R.correlate(frame[None], t, taper=0), 6)
    assert tuple(ip[0]) == d and np.array_equal(s[0], np.float32(d))
    assert abs(float(pk[0]) - 1.0) < 1e-2
    back = R.shift(frame[None], s, fill=np.nan)[0]
    y0, y1, x0, x1 = R.valid_window(s, t.shape)
    assert np.array_equal(back[y0:y1, x0:x1], t[y0:y1, x0:x1]), "the registered frame is frame[p + d]"


def test_ties_go_to_the_lowest_window_index():
    c = np.full((1, 9, 11), 2.5, dtype=np.float32)
    s, ip, pk = R.peak(c, (2, 3))
    assert tuple(ip[0]) == (-2, -3) and pk[0] == 2.5 and np.array_equal(s[0], np.float32([-2, -3])), "constant: den = 0, no refinement"
    c[0, 0, 0], c[0, 8, 9] = 7.0, 7.0                                      # (0, 0) and (-1, -2): the lower index is (-1, -2)
    assert tuple(R.peak(c, (2, 3), subpixel=False)[1][0]) == (-1, -2)
    c[0, 8, 9] = -0.0
    c[0, 0, 0] = 0.0
    c[c == 2.5] = -1.0
    assert tuple(R.peak(c, (2, 3), subpixel=False)[1][0]) == (-1, -2), "-0 and +0 are one value"


def test_window_without_a_finite_value():
    c = np.full((2, 7, 7), np.nan, dtype=np.float32)
    c[1, 3, 3] = 5.0                                                       # outside the window of max_shift 1
    c[0, 0, 0] = -np.inf
    s, ip, pk = R.peak(c, 1)
    assert np.array_equal(s, np.zeros((2, 2), np.float32)) and np.array_equal(ip, np.zeros((2, 2), np.int32)) and np.isnan(pk).all()
    c[1, 0, 1] = -3.0                                                      # one finite value among NaN: it is the peak
    s, ip, pk = R.peak(c, 1)
    assert tuple(ip[1]) == (0, 1) and pk[1] == -3.0 and np.array_equal(s[1], np.float32([0, 1])), "NaN neighbours: delta is 0"


def test_delta_is_guarded_and_clamped():
    assert R.delta(1.0, 2.0, 1.0) == 0.0
    assert R.delta(1.0, 2.0, 1.5) == pytest.approx(0.5 * (1.0 - 1.5) / (1.0 - 4.0 + 1.5))
    assert R.delta(0.0, 1.0, 1.0) == 0.5 and R.delta(1.0, 1.0, 0.0) == -0.5
    assert R.delta(0.0, 1.0, 3.0) == 0.0, "den > 0: not a maximum"
    assert R.delta(1.0, 1.0, 1.0) == 0.0, "den == 0"
    assert R.delta(0.0, 1.0, 1.9999) == 0.5 and R.delta(1.9999, 1.0, 0.0) == -0.5, "clamped"
    assert R.delta(np.nan, 1.0, 0.0) == 0.0 and R.delta(-np.inf, 1.0, 0.0) == 0.0 and R.delta(0.0, np.inf, 0.0) == 0.0


def test_zero_weight_tap_does_not_propagate_a_nan_neighbour():
    x = np.arange(20, dtype=np.float32).reshape(1, 4, 5)
    x[0, 1, 2], x[0, 2, 3], x[0, 0, 0] = np.nan, np.inf, -0.0
    out = R.shift(x, np.float32([[1.0, -2.0]]), fill=-7.0)
    want = np.full((4, 5), -7.0, dtype=np.float32)
    want[0:3, 2:5] = x[0, 1:4, 0:3]
    assert np.array_equal(out[0].view(np.uint32), want.view(np.uint32)), "an integer shift copies bits"
    half = R.shift(x, np.float32([[0.0, 0.5]]))[0]
    assert np.isnan(half[1, 1]) and np.isnan(half[1, 2]) and half[1, 0] == 5.5 and not np.isnan(half[0]).any()
    assert R.shift(x, np.float32([[0.0, 0.0]]))[0].view(np.uint32)[0, 0] == 0x80000000, "-0 survives"
    assert np.array_equal(R.shift(x, np.float32([[np.nan, 0.0]]), fill=3.0)[0], np.full((4, 5), 3.0, np.float32))


@pytest.mark.parametrize("d,want", [(0.5, 0), (-0.5, 0), (1.5, 2), (-1.5, -2), (2.5, 2), (0.75, 1)])
def test_nearest_is_rintf(d, want):
    x = np.arange(12, dtype=np.float32).reshape(1, 1, 12) + 1
    out = R.shift(x, np.float32([[0.0, d]]), mode="nearest")[0, 0]
    ref = np.zeros(12, dtype=np.float32)
    for i in range(12):
        if 0 <= i + want < 12:
            ref[i] = x[0, 0, i + want]
    assert np.array_equal(out, ref)


def test_whitening_the_factors_separately_does_not_overflow():
    F = np.array([[1e11 + 1e11j, 0j, 3 - 4j]], dtype=np.complex64)
    T = np.array([[2e11 - 1e11j, 1 + 1j, 0j]], dtype=np.complex64)
    with np.errstate(all="ignore"):
        prod = F * np.conj(T)
        assert not np.isfinite(prod.real.astype(np.float32) ** 2 + prod.imag.astype(np.float32) ** 2)[0, 0], "the product's |.|^2 overflows"
    Wt = np.conj(R.whiten(T, None, 1e-5))
    out = R.whiten(F, Wt, 1e-5)
    assert np.isfinite(out.view(np.float32)).all() and abs(abs(out[0, 0]) - 1.0) < 2e-6
    assert out[0, 1] == 0 and out[0, 2] == 0, "a zero bin of either factor gives 0"


# ------------------------------------------------------------------------------------------------ the planted scene
@pytest.mark.parametrize("H,W", SIZES)
def test_planted_integer_displacements_are_recovered_exactly(H, W):
    worst = 0.0
    for seed in SEEDS:
        sc = R.scene(seed, H, W)
        c = R.correlate(sc.frames, sc.template, taper=4)
        s, ip, pk = R.peak(c, 6, subpixel=False)
        assert np.array_equal(ip, sc.shifts.astype(np.int32)) and np.array_equal(s, sc.shifts), (H, W, seed)
        for n in range(c.shape[0]):
            m = c[n].copy()
            for a in (-1, 0, 1):
                for b in (-1, 0, 1):
                    m[(ip[n, 0] + a) % H, (ip[n, 1] + b) % W] = -np.inf
            ratio = float(m.max() / pk[n])
            worst = max(worst, ratio)
            assert ratio <= 0.5, f"{H} x {W}, seed {seed}, frame {n}: second peak / peak = {ratio:.3f}"
        reg = R.shift(sc.frames, s, mode="nearest")
        y0, y1, x0, x1 = R.valid_window(s, (H, W))
        assert np.array_equal(reg[:, y0:y1, x0:x1].view(np.uint32), sc.still[:, y0:y1, x0:x1].view(np.uint32)), "an exact crop of the still scene"
    print(f"{H} x {W}: largest second peak / peak = {worst:.3f} (measured 0.391 and 0.208)")


@pytest.mark.parametrize("H,W", SIZES)
def test_planted_subpixel_displacements(H, W):
    worst = 0.0
    for seed in SEEDS:
        sc = R.scene(seed, H, W, subpixel=True)
        s, ip, _ = R.peak(R.correlate(sc.frames, sc.template, taper=4), 6)
        assert np.all(np.abs(ip - sc.shifts) < 1.0), (H, W, seed)       # the floor or the ceiling: near a half either is right
        worst = max(worst, float(np.abs(s - sc.shifts).max()))
    print(f"{H} x {W}: worst sub-pixel error {worst:.4f} px (measured {SUBPIXEL_WORST_MEASURED} over both sizes)")
    assert worst <= SUBPIXEL_BOUND


# ------------------------------------------------------------------------------------------------ the entry points' arguments
def test_reg_window_arguments(L, ptr):
    x, wy, wx, out = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(4))

    def call(x=x, dtype=0, N=2, H=4, W=8, fs=32, wy=wy, wx=wx, out=out):
        return L.cwfa_reg_window(x, dtype, N, H, W, fs, wy, wx, out, None)

    for k in ("x", "wy", "wx", "out"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_window: null" in L.cwfa_last_error()
    assert call(dtype=2) == -1 and call(dtype=-1) == -1 and b"dtype" in L.cwfa_last_error()
    assert call(N=-1) == -2 and call(H=-4) == -2 and call(W=-8) == -2 and b"negative" in L.cwfa_last_error()
    assert call(H=1 << 16, W=1 << 15) == -2 and b"too large" in L.cwfa_last_error()
    assert call(fs=31) == -1 and b"stride" in L.cwfa_last_error()
    assert call(out=x) == -1 and b"must not" in L.cwfa_last_error()
    assert call(N=0) == 0 and call(H=0, fs=0) == 0 and call(W=0, fs=0) == 0, "empty: no launch"


def test_reg_whiten_arguments(L, ptr):
    F, W, out = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(3))

    def call(F=F, W=W, N=2, bins=8, eps=1e-5, out=out):
        return L.cwfa_reg_whiten_c64(F, W, N, bins, eps, out, None)

    assert call(F=None) == -1 and call(out=None) == -1 and b"cwfa_reg_whiten_c64: null" in L.cwfa_last_error()
    assert call(eps=-1.0) == -1 and call(eps=float("inf")) == -1 and call(eps=float("nan")) == -1 and b"eps" in L.cwfa_last_error()
    assert call(N=-1) == -2 and call(bins=-8) == -2 and b"negative" in L.cwfa_last_error()
    for k in ("F", "W", "out"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 4)}) == -3 and b"8-byte" in L.cwfa_last_error(), k
    assert call(W=F) == -1 and call(W=out) == -1 and b"weight plane" in L.cwfa_last_error()
    assert call(N=0) == 0 and call(bins=0) == 0 and call(N=0, W=None, out=F) == 0, "empty: no launch"


def test_reg_peak_arguments(L, ptr):
    c, shifts, ipeak, peak = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(4))

    def call(c=c, N=2, H=5, W=9, fs=45, my=2, mx=4, sub=1, shifts=shifts, ipeak=ipeak, peak=peak):
        return L.cwfa_reg_peak_f32(c, N, H, W, fs, my, mx, sub, shifts, ipeak, peak, None)

    for k in ("c", "shifts", "ipeak", "peak"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_peak_f32: null" in L.cwfa_last_error()
    assert call(sub=2) == -1 and call(sub=-1) == -1 and b"subpixel" in L.cwfa_last_error()
    assert call(N=-1) == -2 and call(H=-5) == -2 and call(my=-1) == -2 and call(mx=-1) == -2 and b"negative" in L.cwfa_last_error()
    assert call(my=3) == -2 and call(mx=5) == -2 and b"wider than" in L.cwfa_last_error(), "2 m + 1 <= the frame"
    assert call(my=1 << 30) == -2, "no overflow in 2 m + 1"
    assert call(fs=44) == -1 and b"stride" in L.cwfa_last_error()
    assert call(shifts=ctypes.c_void_p(shifts.value + 4)) == -3 and call(ipeak=ctypes.c_void_p(ipeak.value + 4)) == -3
    assert b"8-byte" in L.cwfa_last_error()
    assert call(N=0) == 0 and call(H=0, fs=0, my=0) == 0 and call(W=0, fs=0, mx=0) == 0, "empty: no launch"


def test_reg_shift_arguments(L, ptr):
    x, shifts, out = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(3))

    def call(x=x, dtype=0, N=2, H=4, W=8, fs=32, shifts=shifts, mode=0, fill=0.0, out=out):
        return L.cwfa_reg_shift(x, dtype, N, H, W, fs, shifts, mode, fill, out, None)

    for k in ("x", "shifts", "out"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_shift: null" in L.cwfa_last_error()
    assert call(dtype=2) == -1 and b"dtype" in L.cwfa_last_error()
    assert call(mode=2) == -1 and call(mode=-1) == -1 and b"mode" in L.cwfa_last_error()
    assert call(N=-1) == -2 and call(H=-1) == -2 and call(W=-1) == -2 and b"negative" in L.cwfa_last_error()
    assert call(H=1 << 16, W=1 << 15) == -2 and b"too large" in L.cwfa_last_error()
    assert call(fs=31) == -1 and call(fs=-33) == -1 and b"stride" in L.cwfa_last_error(), "a stride that frames overlap under"
    assert call(shifts=ctypes.c_void_p(shifts.value + 4)) == -3 and b"8-byte" in L.cwfa_last_error()
    assert call(out=x) == -1 and b"alias" in L.cwfa_last_error()
    assert call(N=0) == 0 and call(H=0, fs=0) == 0 and call(W=0, fs=0) == 0, "empty: no launch"


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_python_layer_refuses_before_any_device_work():
    from cwfa_amd import ops
    from cwfa_amd.XLFMDataset import estimate_shifts, register_frames, shift_frames, valid_window
    s = torch.zeros(4, 40, 48)
    t = torch.zeros(40, 48)
    sh = torch.zeros(4, 2)
    for call in (lambda: estimate_shifts(s[:, :, ::2], t[:, ::2]), lambda: register_frames(s[:, ::2]), lambda: shift_frames(s[:, :, ::2], sh),
                 lambda: estimate_shifts(s[0], t), lambda: register_frames(s[0]), lambda: shift_frames(s[0], sh)):
        with pytest.raises(ValueError, match=r"contiguous \[N,H,W\]"):
            call()
    for bad in (torch.zeros(40, 47), torch.zeros(1, 40, 48), torch.zeros(40, 48, dtype=torch.float64)):
        with pytest.raises(ValueError, match="template"):
            estimate_shifts(s, bad)
        with pytest.raises(ValueError, match="template"):
            register_frames(s, bad)
    with pytest.raises(ValueError, match="alias"):
        shift_frames(s, sh, out=s)
    with pytest.raises(ValueError, match="alias"):
        shift_frames(s, sh, out=s[:])
    with pytest.raises(ValueError, match="alias"):
        register_frames(s, t, out=s)
    for n_iter in (0, -1):
        with pytest.raises(ValueError, match="n_iter"):
            register_frames(s, t, n_iter=n_iter)
    with pytest.raises(ValueError, match="max_shift"):
        estimate_shifts(s, t, max_shift=20)
    with pytest.raises(ValueError, match="max_shift"):
        estimate_shifts(s, t, max_shift=(3, -1))
    with pytest.raises(ValueError, match="taper"):
        estimate_shifts(s, t, taper=21)
    with pytest.raises(ValueError, match="mode"):
        shift_frames(s, sh, mode="cubic")
    with pytest.raises(ValueError, match="mode"):
        register_frames(s, t, mode="cubic")
    with pytest.raises(ValueError, match="shifts"):
        shift_frames(s, torch.zeros(3, 2))
    for call in (lambda: estimate_shifts(s, t), lambda: shift_frames(s, sh), lambda: register_frames(s, t), lambda: ops.reg_window(s, t[:, 0], t[0]),
                 lambda: ops.reg_peak(s, 2), lambda: ops.reg_shift(s, sh), lambda: ops.reg_whiten(torch.zeros(3, dtype=torch.complex64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_valid_window_is_the_box_every_registered_frame_covers():
    from cwfa_amd.XLFMDataset import valid_window
    assert valid_window(torch.zeros(3, 2), (10, 12)) == (0, 10, 0, 12)
    assert valid_window(torch.tensor([[2.0, -3.0], [-1.0, 1.0]]), (10, 12)) == (1, 8, 3, 11)
    assert valid_window(torch.tensor([[0.25, -0.25]]), (10, 12)) == (0, 9, 1, 12), "a fractional shift reads one pixel further"
    assert valid_window(torch.tensor([[float("nan"), 0.0]]), (10, 12)) == (0, 0, 0, 0)
    assert valid_window(torch.tensor([[10.0, 0.0]]), (10, 12)) == (0, 0, 0, 0)
    for seed in range(3):
        s = np.random.default_rng(seed).uniform(-5, 5, size=(6, 2)).astype(np.float32)
        assert valid_window(torch.from_numpy(s), (20, 30)) == R.valid_window(s, (20, 30))


def test_from_tensors_has_a_registering_form():
    import inspect
    from cwfa_amd.XLFMDataset import XLFMDatasetFull
    p = inspect.signature(XLFMDatasetFull.from_tensors_registered).parameters
    assert list(p) == ["raw_frames", "vols", "img_shape", "ds_id", "register", "sparse"]
    assert p["register"].default is True and p["sparse"].default is None
