"""GPU: rigid frame registration.  The four kernels bit for bit against the numpy restatement
tests/register_ref.py on the SAME inputs -- spectra and correlation maps are handed in, so no FFT difference enters -- at the
smallest shapes that reach every path (one pixel, odd sizes on the element path, the 16-byte path, a frame stride, a base that breaks
16-byte alignment); then ``register_frames`` end to end on the planted scene, where an integer displacement is recovered exactly and
undone bit for bit, which makes ``extract_sparse`` of the registered stack the ``extract_sparse`` of the still scene."""
import functools

import numpy as np
import pytest
import torch

import register_ref as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": (np.float32, torch.float32), "fp16": (np.float16, torch.float16)}
# (N, H, W, unused elements behind every frame, elements in front of the first frame)
LAYOUTS = [(1, 1, 1, 0, 0), (3, 5, 7, 0, 0), (2, 37, 45, 0, 0), (8, 64, 96, 0, 0), (2, 37, 45, 5, 0), (3, 16, 24, 8, 0), (3, 16, 24, 3, 0),
           (3, 16, 24, 0, 1), (2, 5, 7, 2, 3), (2, 6, 20, 0, 0), (2, 6, 20, 4, 2)]   # W = 20: four fp16 pixels per thread in the resampling
SIZES = ((37, 45), (64, 96))


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    if a.dtype == np.complex64:
        a = a.view(np.float32)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def same_values(a, b):
    """Bit for bit where the reference is a number, NaN where it is NaN (the sign and payload of a NaN that an operation made --
    inf - inf -- are the processor's)."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def device_stack(x, pad=0, offset=0, gap=3e4):
    """x [N, ...] (numpy) on the device as a view with ``pad`` unused elements behind every frame, starting ``offset`` elements
    into its buffer; the gaps hold a large value that nothing may read."""
    N, P = x.shape[0], int(np.prod(x.shape[1:]))
    fs = P + pad
    t = torch.from_numpy(np.array(x))
    buf = torch.full((offset + N * fs,), gap, dtype=t.dtype, device="cuda")
    inner, acc = [], 1
    for s in reversed(x.shape[1:]):
        inner.insert(0, acc)
        acc *= s
    view = buf.as_strided(x.shape, (fs, *inner), offset)
    view.copy_(t)
    assert view.data_ptr() == buf.data_ptr() + offset * buf.element_size()
    return view


def stack_data(N, H, W, dt, specials=True):
    rng = np.random.default_rng(17 + 1000 * N + 10 * H + W)
    x = (rng.standard_normal((N, H, W)) * 100.0 + 300.0).astype(DTYPES[dt][0])
    if specials and H * W >= 35:
        x[0, 1, 2], x[0, 2, 3], x[N - 1, H - 1, W - 1], x[0, 0, 0], x[0, 3, 1] = np.nan, np.inf, -np.inf, -0.0, 0.0
    return x


# ------------------------------------------------------------------------------------------------ the window
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N,H,W,pad,offset", LAYOUTS)
def test_window_bit_for_bit(N, H, W, pad, offset, dt):
    from cwfa_amd import ops
    x = stack_data(N, H, W, dt, specials=False)
    wy, wx = R.taper_window(H, min(4, H // 2)), R.taper_window(W, min(4, W // 2))
    want = R.window(x, wy, wx)
    got = ops.reg_window(device_stack(x, pad, offset), torch.from_numpy(wy).cuda(), torch.from_numpy(wx).cuda())
    assert got.dtype == torch.float32 and same_bits(got, want)
    out = torch.empty(N, H, W, device="cuda")
    assert ops.reg_window(device_stack(x, pad, offset), torch.from_numpy(wy).cuda(), torch.from_numpy(wx).cuda(), out=out) is out and same_bits(out, want)
    ones = ops.reg_window(device_stack(x, pad, offset), torch.ones(H, device="cuda"), torch.ones(W, device="cuda"))
    assert same_bits(ones, x.astype(np.float32)), "taper 0: the widened stack"


def test_window_with_an_unaligned_window_vector():
    from cwfa_amd import ops
    x = stack_data(2, 8, 16, "fp32", specials=False)
    wy, wx = R.taper_window(8, 3), R.taper_window(16, 5)
    wxd = device_stack(wx[None], 0, 1, gap=9.0)[0]                          # wx at a 4-byte offset: the element path
    assert same_bits(ops.reg_window(torch.from_numpy(x).cuda(), torch.from_numpy(wy).cuda(), wxd), R.window(x, wy, wx))


# ------------------------------------------------------------------------------------------------ the whitening
def spectra(N, H, Wb, seed=0):
    rng = np.random.default_rng(seed + 100 * N + 10 * H + Wb)
    mag = 10.0 ** rng.uniform(-12, 12, size=(N, H, Wb))
    ph = rng.uniform(0, 2 * np.pi, size=(N, H, Wb))
    F = (mag * np.exp(1j * ph)).astype(np.complex64)
    F[0, 0, 0] = 0
    if H * Wb >= 12:
        F[N - 1, H - 1, Wb - 1] = 0
        F[0, 1, 1] = 1e11 + 1e11j                                          # with the same bin of the plane: |product|^2 overflows
        F[0, 2, 1] = np.complex64(3e-3 - 0j)
    return F


@pytest.mark.parametrize("N,H,W,offset", [(1, 1, 1, 0), (3, 5, 7, 0), (2, 37, 45, 0), (8, 64, 96, 0), (3, 5, 7, 1), (5, 16, 24, 1)])
def test_whiten_bit_for_bit(N, H, W, offset):
    from cwfa_amd import ops
    Wb = W // 2 + 1
    F, T = spectra(N, H, Wb), spectra(1, H, Wb, seed=5)[0]
    if H * Wb >= 12:
        T[1, 1] = 2e11 - 1e11j
        with np.errstate(all="ignore"):
            p = F[0, 1, 1] * np.conj(T[1, 1])
            assert np.isinf(np.float32(p.real) ** 2 + np.float32(p.imag) ** 2), "whitening the product would overflow here"
    eps = 1e-5
    U = R.whiten(T, None, eps)
    Wt = np.conj(U)
    Wt[0, 0] = 0
    Fd = lambda: device_stack(F, 0, offset)
    Wd = device_stack(Wt[None], 0, offset)[0]
    assert same_bits(ops.reg_whiten(device_stack(T[None], 0, offset)[0], None, eps), U), "without a plane: the host's way to Wt"
    assert same_bits(ops.reg_whiten(Fd(), None, eps), R.whiten(F, None, eps))
    want = R.whiten(F, Wt, eps)
    assert np.isfinite(want.view(np.float32)).all()
    src = Fd()
    got = ops.reg_whiten(src, Wd, eps)
    assert same_bits(got, want) and same_bits(src, F), "out of place: F is left alone"
    out = torch.empty_like(got)
    assert ops.reg_whiten(src, Wd, eps, out=out) is out and same_bits(out, want)
    assert ops.reg_whiten(src, Wd, eps, out=src) is src and same_bits(src, want), "in place"
    assert same_bits(ops.reg_whiten(Fd(), Wd, 0.5), R.whiten(F, Wt, 0.5)), "another eps"
    assert complex(got[0, 0, 0]) == 0 and complex(ops.reg_whiten(Fd(), None, eps)[0, 0, 0]) == 0, "a zero bin gives 0"


# ------------------------------------------------------------------------------------------------ the peak
def corr_maps(N, H, W, kind, my, mx):
    rng = np.random.default_rng(3 + 100 * N + 10 * H + W + 7 * my + mx)
    c = (0.05 * rng.standard_normal((N, H, W))).astype(np.float32)
    big = np.float32(0.8)
    for n in range(N):
        if kind == "random":
            continue
        if kind == "wrap":                                                  # negative shifts: the far side of the map
            sy, sx = -min(my, 1 + n % 2), -min(mx, 1 + n % 3)
        elif kind == "border":                                              # on the window's border: a parabola neighbour lies outside
            sy, sx = (my, -mx) if n % 2 == 0 else (-my, mx)
        else:
            sy, sx = 0, 0
        y, x = sy % H, sx % W
        if kind == "plateau":
            c[n] = np.float32(0.25)
            if H * W > 1 and n % 2:
                c[n, (-my) % H, (mx) % W] = np.float32(0.25)
                c[n, 0, 0] = -0.0
        elif kind == "specials":
            c[n] = rng.choice(np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.3, -0.7, 0.3]), size=(H, W),
                              p=[0.3, 0.02 * (n % 2), 0.1, 0.15, 0.15, 0.1, 0.08 + 0.02 * (1 - n % 2), 0.1])
        elif kind == "nan":
            c[n] = np.nan
            if n % 2 and H * W > 1:
                c[n, (my + 1) % H, 0] = -np.inf
        else:
            c[n, y, x] = big
            c[n, (y + 1) % H, x] += np.float32(0.3)                          # uneven neighbours: a delta away from 0
            c[n, y, (x - 1) % W] += np.float32(0.45)
    return c


PEAK_SHAPES = [(1, 1, 1, 0, 0), (3, 5, 7, 0, 0), (2, 37, 45, 0, 0), (8, 64, 96, 0, 0), (2, 37, 45, 5, 0), (3, 16, 24, 0, 1)]


@pytest.mark.parametrize("kind", ["random", "wrap", "border", "plateau", "specials", "nan"])
@pytest.mark.parametrize("N,H,W,pad,offset", PEAK_SHAPES)
def test_peak_bit_for_bit(N, H, W, pad, offset, kind):
    from cwfa_amd import ops
    windows = {(0, 0), (min(2, (H - 1) // 2), min(3, (W - 1) // 2)), ((H - 1) // 2, (W - 1) // 2)}
    for my, mx in sorted(windows):
        c = corr_maps(N, H, W, kind, my, mx)
        cd = device_stack(c, pad, offset, gap=9.0)
        for sub in (True, False):
            ws, wi, wp = R.peak(c, (my, mx), sub)
            s, i, p = ops.reg_peak(cd, (my, mx), sub)
            what = f"{kind} {N}x{H}x{W} window ({my}, {mx}) subpixel {sub}"
            assert np.array_equal(i.cpu().numpy(), wi), what
            assert same_bits(s, ws) and same_bits(p, wp), what
            if not sub:
                assert np.array_equal(s.cpu().numpy(), wi.astype(np.float32)), "the integer peak as fp32"
        assert all(same_bits(a, b) for a, b in zip(ops.reg_peak(cd, (my, mx), True), ops.reg_peak(cd, (my, mx), True))), "two runs, bitwise"
    if kind == "border" and H >= 5 and W >= 7:
        ws, wi, _ = R.peak(corr_maps(N, H, W, kind, 2, 3), (2, 3), True)
        assert np.all(np.abs(wi[:, 0]) == 2) and np.all(np.abs(wi[:, 1]) == 3) and np.any(ws != wi), "refined from outside the window"


def test_peak_accepts_an_int_and_writes_into_out():
    from cwfa_amd import ops
    c = corr_maps(4, 16, 24, "wrap", 3, 3)
    out = (torch.empty(6, 2, device="cuda")[1:5], torch.empty(6, 2, dtype=torch.int32, device="cuda")[1:5], torch.empty(6, device="cuda")[1:5])
    got = ops.reg_peak(torch.from_numpy(c).cuda(), 3, out=out)
    assert all(a is b for a, b in zip(got, out))
    assert all(same_bits(a, b) for a, b in zip(got, R.peak(c, 3)))


def test_more_frames_than_a_grid_axis_holds():
    """N = 70 000 maps of 1 x 4, more than a grid's y or z axis holds and more than the 65 536 workgroups the volumes' peak kernel
    launches: every frame gets its peak, the last one included.  Dense, and with a frame stride larger than the frame: the frame
    index, the item stride and the stride of the two-component outputs together."""
    from cwfa_amd import ops
    N = 70000
    c = np.random.default_rng(5).standard_normal((N, 1, 4)).astype(np.float32)
    win = c[:, 0, [3, 0, 1]]                                                # the window reads x = 3, 0, 1: shifts -1, 0, 1
    wi = np.argmax(win, axis=1)                                             # the first maximum: the lowest index
    want_i = np.stack([np.zeros(N), wi - 1], axis=1).astype(np.int32)
    for cd in (device_stack(c), device_stack(c, pad=3, offset=1, gap=9.0)):
        s, i, p = ops.reg_peak(cd, (0, 1), subpixel=False)
        assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(s.cpu().numpy(), want_i.astype(np.float32))
        assert same_bits(p, win[np.arange(N), wi]), "every frame, the last one included"


# ------------------------------------------------------------------------------------------------ the resampling
def integer_shift_reference(x, d, fill):
    out = np.full(x.shape, fill, dtype=x.dtype)
    N, H, W = x.shape
    for n in range(N):
        dy, dx = int(d[n][0]), int(d[n][1])
        y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        if y1 > y0 and x1 > x0:
            out[n, y0:y1, x0:x1] = x[n, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N,H,W,pad,offset", LAYOUTS)
def test_integer_shifts_copy_bits(N, H, W, pad, offset, dt):
    from cwfa_amd import ops
    x = stack_data(N, H, W, dt)
    rng = np.random.default_rng(N + H + W)
    d = rng.integers(-min(3, H), min(3, H) + 1, size=(N, 2)).astype(np.float32)
    d[0] = 0
    d[N - 1] = (-0.0, 1.0 if W > 1 else 0.0)
    xd = device_stack(x, pad, offset)
    for fill in (0.0, -7.5):
        want = integer_shift_reference(x, d, fill)
        for mode in ("bilinear", "nearest"):
            got = ops.reg_shift(xd, torch.from_numpy(d).cuda(), mode=mode, fill=fill)
            assert got.dtype == DTYPES[dt][1] and same_bits(got, want), (mode, fill)
            assert same_bits(R.shift(x, d, mode, fill), want), "the restatement agrees"
    near = d + np.float32(0.25) * np.float32(rng.choice([-1, 1], size=d.shape))
    assert same_bits(ops.reg_shift(xd, torch.from_numpy(near).cuda(), mode="nearest", fill=-7.5), integer_shift_reference(x, d, -7.5))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N,H,W,pad,offset", LAYOUTS)
def test_fractional_shifts_bit_for_bit(N, H, W, pad, offset, dt):
    from cwfa_amd import ops
    x = stack_data(N, H, W, dt)
    xd = device_stack(x, pad, offset)
    table = np.float32([[0.5, 0.5], [-0.5, 1.5], [0.0, 0.25], [-1.75, 0.0], [2.3, -3.6], [-0.001, 0.999], [float(H), 0.4], [0.3, -float(W) - 2.5],
                        [np.nan, 0.0], [0.5, np.inf], [1e30, -1e30], [1.0, 0.5], [0.5, -2.0], [-0.5, -0.5], [1e-30, 1e-30], [3e9, 0.5]])
    for k in range(0, len(table), max(N, 1)):
        d = np.resize(table[k:k + N], (N, 2)).astype(np.float32)
        for mode in ("bilinear", "nearest"):
            for fill in (0.0, 2.5):
                want = R.shift(x, d, mode, fill)
                got = ops.reg_shift(xd, torch.from_numpy(d).cuda(), mode=mode, fill=fill)
                assert got.dtype == DTYPES[dt][1] and same_values(got, want), (d.tolist(), mode, fill)
    out = torch.empty(N, H, W, dtype=DTYPES[dt][1], device="cuda")
    d = np.resize(table[:N], (N, 2)).astype(np.float32)
    assert ops.reg_shift(xd, torch.from_numpy(d).cuda(), out=out) is out and same_values(out, R.shift(x, d))


def test_shift_refuses_aliasing_and_bad_arguments():
    from cwfa_amd import ops
    x = torch.zeros(2, 8, 8, device="cuda")
    s = torch.zeros(2, 2, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        ops.reg_shift(x, s, out=x)
    with pytest.raises(ValueError, match="alias"):
        ops.reg_window(x, x[0, 0], x[0, 0], out=x)
    with pytest.raises(ValueError, match="mode"):
        ops.reg_shift(x, s, mode="cubic")
    with pytest.raises(ValueError, match="max_shift"):
        ops.reg_peak(x, 4)
    with pytest.raises(ValueError, match="shifts"):
        ops.reg_shift(x, s[:1])


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def planted(seed, H, W, subpixel=False, rest=0):
    return R.scene(seed, H, W, subpixel=subpixel, rest=rest)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("H,W", SIZES)
def test_integer_displacements_are_undone_bit_for_bit(H, W, seed):
    from cwfa_amd.XLFMDataset import extract_sparse, register_frames, valid_window
    sc = planted(seed, H, W)
    frames, still, template = (torch.from_numpy(a).cuda() for a in (sc.frames, sc.still, sc.template))
    reg = register_frames(frames, template, max_shift=6, taper=4, subpixel=False, mode="nearest")
    assert np.array_equal(reg.shifts.cpu().numpy(), sc.shifts), "exactly the planted displacements"
    assert reg.template is template and reg.frames.dtype == torch.float32 and tuple(reg.peak.shape) == (sc.frames.shape[0],)
    y0, y1, x0, x1 = valid_window(reg.shifts, (H, W))
    assert (y0, y1, x0, x1) == R.valid_window(sc.shifts, (H, W)) and y1 - y0 >= H - 8 and x1 - x0 >= W - 8
    crop = lambda t: t[:, y0:y1, x0:x1].contiguous()
    assert same_bits(crop(reg.frames), sc.still[:, y0:y1, x0:x1]), "the registered stack is the still scene"
    a, b, moved = extract_sparse(crop(reg.frames), noise_k=2.0), extract_sparse(crop(still), noise_k=2.0), extract_sparse(crop(frames), noise_k=2.0)
    for k in ("sparse", "baseline", "scales", "tau"):
        assert same_bits(getattr(a, k), getattr(b, k)), f"extract_sparse of the registered crop: {k}"
    assert not same_bits(moved.sparse, b.sparse) and not same_bits(moved.baseline, b.baseline), "the unregistered stack does not"
    bil = register_frames(frames, template, max_shift=6, taper=4, subpixel=False)
    assert same_bits(bil.frames, reg.frames), "an integer shift: bilinear copies bits too"
    half = register_frames(frames.half(), template, max_shift=6, taper=4, subpixel=False, mode="nearest")
    assert half.frames.dtype == torch.float16 and np.array_equal(half.shifts.cpu().numpy(), sc.shifts)
    assert same_bits(crop(half.frames), sc.still.astype(np.float16)[:, y0:y1, x0:x1])


# The largest |device - restatement| of the sub-pixel shifts over SIZES x seeds 0 .. 2, observed on the MI355X: 4.768e-07 px at
# either size -- one unit in the last place of an fp32 shift between 4 and 8.  The two differ only in the transforms (rocFFT in fp32
# against numpy.fft in float64), whose rounding reaches the shift through the parabola's denominator.  The bound is 4 x the
# observation, as the feature's specification sets it.
OBSERVED_SUBPIXEL_DIFF = 4.768e-07
SUBPIXEL_DIFF_BOUND = 4.0 * OBSERVED_SUBPIXEL_DIFF


@pytest.mark.parametrize("H,W", SIZES)
def test_subpixel_shifts_against_the_restatement(H, W):
    from cwfa_amd.XLFMDataset import estimate_shifts
    worst = 0.0
    for seed in (0, 1, 2):
        sc = planted(seed, H, W, True)
        want, wpk = R.estimate_shifts(sc.frames, sc.template, 6, 4)
        got, pk = estimate_shifts(torch.from_numpy(sc.frames).cuda(), torch.from_numpy(sc.template).cuda(), max_shift=6, taper=4)
        got = got.cpu().numpy()
        worst = max(worst, float(np.abs(got - want).max()))
        _, wi, _ = R.peak(R.correlate(sc.frames, sc.template, 4), 6, False)
        assert np.all(np.abs(got - wi) <= 0.5), "the same integer peak: the refinement moves it by at most half a pixel"
        assert float(np.abs(pk.cpu().numpy() - wpk).max()) < 1e-3
    print(f"{H} x {W}: largest |device - restatement| of the sub-pixel shifts = {worst:.3e} px")
    assert worst <= SUBPIXEL_DIFF_BOUND


# The stack's own median as template: with few frames, a frame's own noise survives in the median wherever the frame is the median
# value and correlates with itself at shift 0.  The restatement shows it (8 frames, all moved: every estimate is 0); it recovers
# the planted displacements, second peak / peak <= 0.32, where most frames rest (6 of 8 here) and the Gaussian low-pass of 0.75 px
# takes the noise band down.  That scene is tested; DESIGN.md section 26 records the limit.
MEDIAN_KW = dict(max_shift=6, taper=4, smooth=0.75, subpixel=False, mode="nearest")


@pytest.mark.parametrize("H,W", SIZES)
def test_two_iterations_from_the_stack_own_median(H, W):
    from cwfa_amd.XLFMDataset import register_frames
    sc = planted(0, H, W, rest=5)
    frames = torch.from_numpy(sc.frames).cuda()
    reg = register_frames(frames, None, n_iter=2, **MEDIAN_KW)
    s = reg.shifts.cpu().numpy()
    assert np.array_equal(s - s[0], sc.shifts - sc.shifts[0]), "the planted displacements up to the median template's common offset"
    assert tuple(reg.template.shape) == (H, W) and reg.template.dtype == torch.float32
    one = register_frames(frames, None, n_iter=1, **MEDIAN_KW)
    assert not same_bits(one.template, reg.template), "the second template is the registered stack's median"
    assert same_bits(reg.template, R.lower_median(one.frames.cpu().numpy())), "... of the FIRST pass, and the frames are the originals moved once"
    assert same_bits(reg.frames, R.shift(sc.frames, s, "nearest"))
    again = register_frames(frames, None, n_iter=2, **MEDIAN_KW)
    assert same_bits(again.frames, reg.frames) and same_bits(again.shifts, reg.shifts) and same_bits(again.peak, reg.peak)


def test_dataset_registers_before_the_sparse_stage():
    from cwfa_amd.XLFMDataset import XLFMDatasetFull, extract_sparse, prepare_frames, register_frames
    sc = planted(1, 64, 96, rest=5)
    raw = torch.from_numpy(sc.frames).cuda()
    img_shape = (48, 48)
    kw = dict(MEDIAN_KW)
    prepared = prepare_frames(raw, img_shape)
    reg = register_frames(prepared, **kw)
    by_hand = extract_sparse(reg.frames.clone(), noise_k=1.0).sparse
    ds = XLFMDatasetFull.from_tensors_registered(raw, None, img_shape, "x", register=kw, sparse=dict(noise_k=1.0))
    assert same_bits(ds.stacked_views, by_hand) and same_bits(ds.registration.shifts, reg.shifts) and ds.registration.frames is None
    assert same_bits(XLFMDatasetFull.from_tensors_registered(raw, None, img_shape, register=kw).stacked_views, reg.frames)
    pair = XLFMDatasetFull.from_tensors_registered(raw, None, img_shape, register=kw, sparse=dict(pair=True))
    assert tuple(pair.stacked_views.shape) == (8, 48, 48, 2) and same_bits(pair.stacked_views[..., 0], reg.frames)
    assert bool((reg.shifts != 0).any()) and not same_bits(reg.frames, prepared), "something moved"
    today = XLFMDatasetFull.from_tensors(raw, None, img_shape, "x", sparse=True)
    for register in (None, False):
        same = XLFMDatasetFull.from_tensors_registered(raw, None, img_shape, "x", register=register, sparse=True)
        assert same_bits(same.stacked_views, today.stacked_views) and not hasattr(same, "registration")
    assert same_bits(XLFMDatasetFull.from_tensors(raw, None, img_shape).stacked_views, prepared), "from_tensors itself: today's bits"
