"""GPU: per-lenslet frame registration.  The four new kernels bit for bit against the numpy restatement
tests/register_views_ref.py on the SAME inputs, at the smallest shapes that reach every path (one pixel, boxes over every border of
the frame and outside it, odd view widths on the element path, the 16-byte path, a frame stride, a base that breaks 16-byte
alignment, 254 views, label boundaries inside a thread's pixel group); then ``register_views`` end to end on the planted lenslet
scene, where every per-view displacement is recovered exactly and undone bit for bit, and where ``register_frames`` cannot do it."""
import functools

import numpy as np
import pytest
import torch

import register_ref as R
import register_views_ref as V
from test_gpu_register import DTYPES, LAYOUTS, device_stack, same_bits, same_values, stack_data
from test_register_views_cpu import LABEL_CASES, planted_shifts

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def scene(seed, subpixel=False):
    return V.lenslet_scene(seed, subpixel=subpixel)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_tensors(a, b):
    """``same_bits`` for device tensors, bytes included."""
    return torch.equal(a, b) if a.dtype == torch.uint8 else same_bits(a, b)


# ------------------------------------------------------------------------------------------------ the views
BORDERS = [[0, 5], [11, 5], [5, 0], [5, 15], [0, 0], [11, 15], [-20, -20], [6, 40], [6, 8]]   # over every border, two outside, one inside
# (N, H, W, centres or their number, ph, pw, unused elements behind every frame, elements in front of the first)
VIEW_CASES = [(1, 1, 1, [[0, 0]], 1, 1, 0, 0), (2, 9, 11, 3, 4, 6, 0, 0), (3, 37, 45, 4, 8, 8, 0, 0), (2, 12, 16, BORDERS, 4, 8, 0, 0),
              (2, 12, 16, BORDERS, 4, 6, 0, 0), (2, 12, 16, BORDERS, 5, 8, 5, 0), (3, 12, 16, BORDERS, 4, 8, 3, 1), (2, 9, 11, 3, 3, 5, 0, 0),
              (2, 9, 11, 3, 4, 4, 2, 3), (2, 16, 16, 254, 1, 1, 0, 0), (1, 192, 192, "scene", 48, 48, 0, 0)]


def view_centres(spec, H, W):
    if isinstance(spec, list):
        return np.int32(spec)
    if spec == "scene":
        return V.CENTERS.copy()
    rng = np.random.default_rng(spec + H + W)
    return np.stack([rng.integers(-2, H + 2, size=spec), rng.integers(-2, W + 2, size=spec)], axis=1).astype(np.int32)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N,H,W,spec,ph,pw,pad,offset", VIEW_CASES)
def test_window_views_bit_for_bit(N, H, W, spec, ph, pw, pad, offset, dt):
    from cwfa_amd import ops
    x = stack_data(N, H, W, dt, specials=False)
    c = view_centres(spec, H, W)
    wy, wx = R.taper_window(ph, min(2, ph // 2)), R.taper_window(pw, min(2, pw // 2))
    want = V.window_views(x, c, (ph, pw), wy, wx)
    got = ops.reg_window_views(device_stack(x, pad, offset), c, (ph, pw), cuda(wy), cuda(wx))
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, len(c), ph, pw) and same_bits(got, want)
    out = torch.full((N, len(c), ph, pw), 7.0, device="cuda")
    assert ops.reg_window_views(device_stack(x, pad, offset), torch.from_numpy(c), [ph, pw], cuda(wy), cuda(wx), out=out) is out and same_bits(out, want)
    ones = ops.reg_window_views(device_stack(x, pad, offset), c, (ph, pw), torch.ones(ph, device="cuda"), torch.ones(pw, device="cuda"))
    assert same_bits(ones, V.cut_views(x, c, (ph, pw)).astype(np.float32)), "taper 0: the widened views, +0 outside the frame"


def test_window_views_into_an_unaligned_out_and_no_frames():
    from cwfa_amd import ops
    x = stack_data(2, 12, 16, "fp32", specials=False)
    c, wy, wx = np.int32(BORDERS), R.taper_window(4, 1), R.taper_window(8, 2)
    out = device_stack(np.zeros((2, len(c), 4, 8), dtype=np.float32), 0, 1, gap=9.0)      # pw % 4 == 0, the base is not 16-byte aligned
    assert ops.reg_window_views(cuda(x), c, (4, 8), cuda(wy), cuda(wx), out=out) is out and same_bits(out, V.window_views(x, c, (4, 8), wy, wx))
    none = ops.reg_window_views(torch.empty(0, 12, 16, device="cuda"), c, (4, 8), cuda(wy), cuda(wx))
    assert tuple(none.shape) == (0, len(c), 4, 8)
    whole = torch.zeros(2, 12, 16, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        ops.reg_window_views(whole, [[6, 8]], (12, 16), torch.ones(12, device="cuda"), torch.ones(16, device="cuda"), out=whole.reshape(2, 1, 12, 16))


# ------------------------------------------------------------------------------------------------ the label map
@pytest.mark.parametrize("case", list(LABEL_CASES) + ["scene", "many"])
def test_label_map_bit_for_bit(case):
    from cwfa_amd.XLFMDataset import view_labels
    if case == "scene":
        c, vs, shape = V.CENTERS, (V.VIEW, V.VIEW), V.FRAME
    elif case == "many":
        rng = np.random.default_rng(4)
        c, vs, shape = rng.integers(-3, 40, size=(254, 2)), (7, 4), (37, 45)
    else:
        c, vs, shape = LABEL_CASES[case]
    got = view_labels(shape, c, vs)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), V.label_map(shape, c, vs))


# ------------------------------------------------------------------------------------------------ the fit
def fit_inputs(N, L, seed=0):
    """Planted motion plus noise, a few far outliers, and peaks with NaN, inf, negative values and values around min_peak."""
    rng = np.random.default_rng(seed + 10 * N + L)
    g = rng.integers(-64, 65, size=(L, 2)).astype(np.float64) / 4.0
    d, a = rng.uniform(-3, 3, size=(N, 2)), rng.uniform(-0.1, 0.1, size=N)
    s = d[:, None, :] + a[:, None, None] * g[None] + 0.2 * rng.standard_normal((N, L, 2))
    s = np.where(rng.random((N, L, 1)) < 0.1, s + rng.uniform(-6, 6, size=(N, L, 2)), s).astype(np.float32)
    pk = rng.uniform(0.0, 0.5, size=(N, L))
    pk = np.where(rng.random((N, L)) < 0.1, rng.choice([np.nan, np.inf, -np.inf, -0.2, 0.25, -0.0], size=(N, L)), pk).astype(np.float32)
    if N >= 4:
        pk[1] = np.nan                                                    # m = 0
        pk[2, 1:] = -1.0                                                  # m = 1
        s[3] = np.float32(rng.integers(-4, 5, size=(L, 2))) * 100        # a frame whose rejection pass removes much or all
    return s, pk, g


def check_fit(s, pk, g, **kw):
    from cwfa_amd import ops
    want = V.fit(s, pk, g, **kw)
    got = ops.reg_fit_views(cuda(s), cuda(pk), cuda(g), **kw)
    again = ops.reg_fit_views(cuda(s), cuda(pk), cuda(g), **kw)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float64 and got[2].dtype == torch.uint8
    assert np.array_equal(got[2].cpu().numpy(), want.inlier), kw
    assert same_values(got[1], want.params) and same_values(got[0], want.table), kw
    assert all(same_tensors(a, b) for a, b in zip(got, again)), "two runs, bitwise"
    return want


# L = 1, 7 and 254 at N = 1, and N = 70 000 (past 65 535, more than a thousand workgroups) at L = 1 and 7; 254 views go with 600
# frames: the restatement of 70 000 x 254 alone takes 8 s on the host and reaches no other path of a kernel whose threads are frames
@pytest.mark.parametrize("N,L", [(1, 1), (1, 7), (1, 254), (70000, 1), (70000, 7), (600, 254)])
def test_fit_bit_for_bit(N, L):
    s, pk, g = fit_inputs(N, L)
    want = check_fit(s, pk, g, min_peak=0.25, reject=1.0, model="axial")
    if N > 1:
        assert 0 < want.inlier.mean() < 1 and np.isfinite(want.params).all()
    check_fit(s, pk, g, min_peak=0.0, reject=np.inf, model="free")
    check_fit(s, pk, g, min_peak=0.0, reject=0.5, model="free")


def test_fit_cpu_cases_on_the_device():
    s, d, a, pk = planted_shifts()
    f = check_fit(s, pk, V.G)
    assert np.abs(f.params - np.column_stack([d, a])).max() <= 1e-12
    none = pk.copy()
    none[1], none[2] = np.nan, -0.5
    check_fit(s, none, V.G)
    check_fit(s, none, V.G, model="free")
    one = pk.copy()
    one[0, 1:] = np.inf
    check_fit(s, one, V.G)
    check_fit(s, pk, np.tile(np.float64([[3.0, -2.0]]), (7, 1)), reject=np.inf)
    moved, low = s.copy(), pk.copy()
    moved[0, 3] += 5.0
    moved[1, 4] -= 7.0
    low[0, 3], low[1, 4] = np.nan, 0.2
    check_fit(moved, low, V.G, min_peak=0.25, reject=np.inf)
    check_fit(moved, low, V.G, min_peak=0.2, reject=np.inf)
    check_fit(moved, low, V.G, min_peak=0.0, reject=1.0)
    check_fit(moved, low, V.G, min_peak=0.0, reject=1.0, model="free")
    f = check_fit(np.float32([[[0, 0], [4, 0]]]), np.ones((1, 2), dtype=np.float32), np.float64([[0, -1], [0, 1]]), reject=1.0)
    assert f.inlier.tolist() == [[1, 1]] and f.params.tolist() == [[2.0, 0.0, 0.0]], "everything rejected: the first fit stands"
    off = s.copy()
    off[:, 2, 1] += np.float32(0.25)
    check_fit(off, pk, V.G)
    check_fit(off, pk, V.G, model="free")
    from cwfa_amd import ops
    t, p, i = ops.reg_fit_views(torch.empty(0, 7, 2, device="cuda"), torch.empty(0, 7, device="cuda"), cuda(V.G))
    assert tuple(t.shape) == (0, 8, 2) and tuple(p.shape) == (0, 3) and tuple(i.shape) == (0, 7)


# ------------------------------------------------------------------------------------------------ the labelled resampling
FRACTIONS = np.float32([[0.5, 0.5], [-0.5, 1.5], [0.0, 0.25], [-1.75, 0.0], [2.3, -3.6], [-0.001, 0.999], [40.0, 0.4], [0.3, -100.5],
                        [np.nan, 0.0], [0.5, np.inf], [1e30, -1e30], [1.0, 0.5], [0.5, -2.0], [-0.5, -0.5], [1e-30, 1e-30], [3e9, 0.5]])


def label_maps(H, W, L):
    """Maps with the labels 0 .. L and above: constant along a thread's pixel group, a boundary inside it, and per pixel."""
    rng = np.random.default_rng(H + W + L)
    cols = np.zeros((H, W), dtype=np.uint8)
    cols[:, W // 2:] = 1
    cols[:, min(3, W - 1):min(6, W)] = L + 3                              # a boundary at column 3: inside a group of 4 and of 8
    cols[H // 2:] += 1
    return {"columns": cols, "pixels": rng.integers(0, L + 3, size=(H, W)).astype(np.uint8)}


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N,H,W,pad,offset", LAYOUTS)
def test_a_single_label_is_reg_shift_on_the_device(N, H, W, pad, offset, dt):
    from cwfa_amd import ops
    x = stack_data(N, H, W, dt)
    xd = device_stack(x, pad, offset)
    rng = np.random.default_rng(N + H + W)
    L = 3
    for k in range(0, len(FRACTIONS), max(N, 1)):
        table = rng.uniform(-3, 3, size=(N, L + 1, 2)).astype(np.float32)
        table[:, 2] = np.resize(FRACTIONS[k:k + N], (N, 2))
        lab = torch.full((H, W), 2, dtype=torch.uint8, device="cuda")
        for mode in ("bilinear", "nearest"):
            for fill in (0.0, 2.5):
                want = ops.reg_shift(xd, cuda(table[:, 2]), mode=mode, fill=fill)
                got = ops.reg_shift_labeled(xd, cuda(table), lab, mode=mode, fill=fill)
                assert got.dtype == DTYPES[dt][1] and same_bits(got, want), (table[:, 2].tolist(), mode, fill)
    rest = ops.reg_shift_labeled(xd, cuda(table), torch.full((H, W), 250, dtype=torch.uint8, device="cuda"))
    assert same_bits(rest, ops.reg_shift(xd, cuda(table[:, 3]))), "a label above L reads row L"


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N,H,W,pad,offset", LAYOUTS)
def test_shift_labeled_bit_for_bit(N, H, W, pad, offset, dt):
    from cwfa_amd import ops
    x = stack_data(N, H, W, dt)                                            # NaN, inf, -inf and -0 among the pixels
    xd = device_stack(x, pad, offset)
    rng = np.random.default_rng(2 * N + H + W)
    L = 4
    integer = rng.integers(-min(3, H), min(3, H) + 1, size=(N, L + 1, 2)).astype(np.float32)
    integer[:, 0] = (-0.0, 0.0)
    frac = np.resize(rng.permutation(FRACTIONS), (N, L + 1, 2)).astype(np.float32)
    for name, lab in label_maps(H, W, L).items():
        labd = cuda(lab)
        for mode in ("bilinear", "nearest"):
            want = V.shift_labeled(x, integer, lab, mode, -7.5)
            got = ops.reg_shift_labeled(xd, cuda(integer), labd, mode=mode, fill=-7.5)
            assert got.dtype == DTYPES[dt][1] and same_bits(got, want), ("an integer table copies bits", name, mode)
            for fill in (0.0, 2.5):
                want = V.shift_labeled(x, frac, lab, mode, fill)
                got = ops.reg_shift_labeled(xd, cuda(frac), labd, mode=mode, fill=fill)
                assert same_values(got, want), (name, mode, fill)
    out = torch.empty(N, H, W, dtype=DTYPES[dt][1], device="cuda")
    assert ops.reg_shift_labeled(xd, cuda(frac), labd, out=out) is out and same_values(out, V.shift_labeled(x, frac, lab))


def test_shift_labeled_no_frames_and_refusals():
    from cwfa_amd import ops
    lab = torch.zeros(8, 8, dtype=torch.uint8, device="cuda")
    none = ops.reg_shift_labeled(torch.empty(0, 8, 8, device="cuda"), torch.empty(0, 3, 2, device="cuda"), lab)
    assert tuple(none.shape) == (0, 8, 8)
    x, t = torch.zeros(2, 8, 8, device="cuda"), torch.zeros(2, 3, 2, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        ops.reg_shift_labeled(x, t, lab, out=x)
    with pytest.raises(ValueError, match="mode"):
        ops.reg_shift_labeled(x, t, lab, mode="cubic")
    with pytest.raises(ValueError, match="table"):
        ops.reg_shift_labeled(x, t[:1], lab)
    with pytest.raises(ValueError, match="labels"):
        ops.reg_shift_labeled(x, t, lab[:, :7])


# ------------------------------------------------------------------------------------------------ end to end
KW = dict(max_shift=6, taper=4, subpixel=False, mode="nearest")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_view_displacements_are_undone_bit_for_bit(seed):
    from cwfa_amd.XLFMDataset import extract_sparse, register_frames, register_views, valid_view_windows, view_labels
    sc = scene(seed)
    frames, still, template = cuda(sc.frames), cuda(sc.still), cuda(sc.template)
    reg = register_views(frames, sc.centers, sc.view_shape, template=template, directions=sc.directions, model="axial", **KW)
    assert np.array_equal(reg.shifts.cpu().numpy(), sc.view_shifts), "exactly the planted per-view displacements"
    assert reg.template is template and reg.frames.dtype == torch.float32 and tuple(reg.peak.shape) == (8, 7) and bool(reg.inlier.all())
    want = V.fit(sc.view_shifts, reg.peak.cpu().numpy(), sc.directions)
    assert same_bits(reg.params, want.params) and same_bits(reg.table, want.table), "the restatement's fit of those shifts"
    assert np.abs(reg.params.cpu().numpy() - np.column_stack([sc.d, sc.a])).max() <= 1e-12
    wins = valid_view_windows(reg.table, sc.centers, sc.view_shape, V.FRAME)
    assert np.array_equal(wins, V.valid_view_windows(want.table, sc.centers, sc.view_shape, V.FRAME))
    for y0, y1, x0, x1 in wins:
        assert y1 - y0 >= 40 and x1 - x0 >= 40
        crop = lambda t: t[:, y0:y1, x0:x1].contiguous()
        assert same_bits(crop(reg.frames), sc.still[:, y0:y1, x0:x1]), "the registered views are the still scene"
        a, b = extract_sparse(crop(reg.frames), noise_k=2.0), extract_sparse(crop(still), noise_k=2.0)
        for k in ("sparse", "baseline", "scales", "tau"):
            assert same_bits(getattr(a, k), getattr(b, k)), f"extract_sparse of the registered crop: {k}"
    assert same_bits(reg.frames, V.shift_labeled(sc.frames, want.table, V.label_map(V.FRAME, sc.centers, sc.view_shape), "nearest"))
    # what the feature is for: one vector per frame cannot undo a fan
    rigid = register_frames(frames, template, **KW).frames.cpu().numpy()
    for n in np.nonzero(sc.a)[0]:
        assert not all(np.array_equal(rigid[n, y0:y1, x0:x1], sc.still[n, y0:y1, x0:x1]) for y0, y1, x0, x1 in wins[1:]), "register_frames, off-axis views"
    if seed == 0:
        labels = view_labels(V.FRAME, sc.centers, sc.view_shape)
        for kw in (dict(chunk=3), dict(mode="bilinear"), dict(model="free"), dict(labels=labels)):
            other = register_views(frames, sc.centers, sc.view_shape, template=template, directions=sc.directions, **{**KW, **kw})
            assert same_bits(other.frames, reg.frames) and same_bits(other.table, reg.table), kw
        default = register_views(frames, sc.centers, sc.view_shape, template=template, **KW)           # g = centres - mean = 4 G
        assert np.abs(default.params.cpu().numpy() - np.column_stack([sc.d, sc.a / 4])).max() <= 1e-12 and same_bits(default.frames, reg.frames)


def test_two_iterations_from_the_stack_own_median_run_and_repeat():
    from cwfa_amd.XLFMDataset import register_views
    sc = scene(0)
    frames = cuda(sc.frames)
    kw = dict(directions=sc.directions, n_iter=2, smooth=0.75, **KW)
    a, b = register_views(frames, sc.centers, sc.view_shape, **kw), register_views(frames, sc.centers, sc.view_shape, **kw)
    assert tuple(a.template.shape) == V.FRAME and tuple(a.table.shape) == (8, 8, 2) and tuple(a.params.shape) == (8, 3)
    for k in ("frames", "table", "params", "shifts", "inlier", "template"):
        assert same_tensors(getattr(a, k), getattr(b, k)), k
    one = register_views(frames, sc.centers, sc.view_shape, **{**kw, "n_iter": 1})
    assert same_bits(a.template, R.lower_median(one.frames.cpu().numpy())), "the second template is the first pass's median"
    assert same_bits(a.frames, V.shift_labeled(sc.frames, a.table.cpu().numpy(), V.label_map(V.FRAME, sc.centers, sc.view_shape), "nearest")), "the originals, moved once"


# The bound of tests/test_gpu_register.py for these same kernels: 4 units in the last place of an fp32 shift of this magnitude (the
# planted |shift| is below 4.5 px, the estimates lie in [4, 8) at most: one unit is 2^-21 = 4.768e-07 px).  The restatement and
# the device differ only in the transforms (rocFFT in fp32 against numpy.fft in float64).
SUBPIXEL_DIFF_BOUND = 4.0 * 2.0 ** -21


@pytest.mark.parametrize("subpixel", [True, "dft"])
def test_subpixel_view_shifts_against_the_restatement(subpixel):
    from cwfa_amd.XLFMDataset import estimate_view_shifts
    worst, off = 0.0, 0.0
    for seed in (0, 1):
        sc = scene(seed, True)
        want, wpk = V.estimate_view_shifts(sc.frames, sc.template, sc.centers, sc.view_shape, 6, 4, subpixel=subpixel)
        got, pk = estimate_view_shifts(cuda(sc.frames), cuda(sc.template), sc.centers, sc.view_shape, max_shift=6, taper=4, subpixel=subpixel)
        got = got.cpu().numpy()
        worst = max(worst, float(np.abs(got - want).max()))
        off = max(off, float(np.abs(want - sc.view_shifts).max()))
        assert float(np.abs(pk.cpu().numpy() - wpk).max()) < 1e-3
    print(f"subpixel={subpixel!r}: largest |device - restatement| = {worst:.3e} px (bound {SUBPIXEL_DIFF_BOUND:.3e}); restatement - planted = {off:.4f} px")
    assert off <= 0.5, "no further off than rounding to the nearest integer (section 26.4's rule)"
    assert worst <= SUBPIXEL_DIFF_BOUND
