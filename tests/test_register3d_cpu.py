"""CPU: rigid registration of volumes without a GPU -- the numpy restatement tests/register3d_ref.py checked
against itself and against the 2-D restatement (sign convention, ties and the index order over three axes, NaN, the parabola's
guards per axis, zero-weight planes, nearest, D = 1), planted integer and sub-voxel displacements on the scene, ``valid_box``, the
argument validation of the three entry points through the built library, and the refusals the Python layer decides before any
device work."""
import ctypes

import numpy as np
import pytest
import torch

import register3d_ref as R3
import register_ref as R

# (shape, the largest planted |d| per axis, taper); the search window is one wider than |d| per axis
CASES = (((12, 24, 28), (2, 3, 3), (1, 3, 3)), ((16, 37, 45), (3, 4, 4), (2, 4, 4)))
SEEDS = tuple(range(8))
# MEASURED on this scene over SEEDS, per shape: the largest correlation value outside the 3 x 3 x 3 around the peak over the peak,
# 0.404 and 0.174 (the cap is 0.5: it is what lets the device test demand exact integers although rocFFT and numpy round
# differently); the worst |estimate - planted| of the sub-voxel scene, 0.361 and 0.267 voxels.  Recorded, not tuned: what is
# asserted is that the integer peak is the planted displacement's floor or ceiling and the refined estimate is within 0.5 voxel,
# the worst case of rounding to the nearest integer (the parabola is biased toward the integer, section 26.4).
CAP = 0.5
SUBVOXEL_BOUND = 0.5
u32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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
@pytest.mark.parametrize("d", [(0, 0, 0), (1, 3, -2), (-2, -4, 1), (2, -1, -5)])
def test_sign_convention_template_displaced_by_d_reports_d(d):
    rng = np.random.default_rng(7)
    t = rng.random((8, 14, 18)).astype(np.float32)
    vol = np.roll(t, d, axis=(0, 1, 2))                                    # vol[p] = t[p - d], cyclic: the peak is 1 up to rounding
    s, ip, pk = R3.peak(R3.correlate(vol[None], t, taper=0), (2, 5, 6))
    assert tuple(ip[0]) == d and np.array_equal(s[0], np.float32(d))
    assert abs(float(pk[0]) - 1.0) < 1e-2
    back = R3.shift(vol[None], s, fill=np.nan)[0]
    z0, z1, y0, y1, x0, x1 = R3.valid_box(s, t.shape)
    assert np.array_equal(back[z0:z1, y0:y1, x0:x1], t[z0:z1, y0:y1, x0:x1]), "the registered volume is vol[p + d]"


def test_ties_go_to_the_lowest_window_index_z_slowest():
    c = np.full((1, 5, 9, 11), 2.5, dtype=np.float32)
    s, ip, pk = R3.peak(c, (1, 2, 3))
    assert tuple(ip[0]) == (-1, -2, -3) and pk[0] == 2.5 and np.array_equal(s[0], np.float32([-1, -2, -3])), "constant: den = 0, no refinement"
    c[0, 0, 0, 0], c[0, 4, 2, 3], c[0, 0, 8, 9] = 7.0, 7.0, 7.0           # (0,0,0), (-1,2,3), (0,-1,-2): z is the slowest axis
    assert tuple(R3.peak(c, (1, 2, 3), subpixel=False)[1][0]) == (-1, 2, 3)
    c[0, 4, 2, 3] = 2.5
    assert tuple(R3.peak(c, (1, 2, 3), subpixel=False)[1][0]) == (0, -1, -2), "then y, then x"
    c[0, 0, 8, 9], c[0, 0, 0, 0] = -0.0, 0.0
    c[c == 2.5] = -1.0
    assert tuple(R3.peak(c, (1, 2, 3), subpixel=False)[1][0]) == (0, -1, -2), "-0 and +0 are one value"


def test_window_without_a_finite_value():
    c = np.full((2, 5, 7, 7), np.nan, dtype=np.float32)
    c[1, 2, 3, 3] = 5.0                                                    # outside the window of max_shift 1
    c[0, 0, 0, 0] = -np.inf
    s, ip, pk = R3.peak(c, 1)
    assert np.array_equal(s, np.zeros((2, 3), np.float32)) and np.array_equal(ip, np.zeros((2, 3), np.int32)) and np.isnan(pk).all()
    c[1, 4, 0, 1] = -3.0                                                   # one finite value among NaN: it is the peak
    s, ip, pk = R3.peak(c, 1)
    assert tuple(ip[1]) == (-1, 0, 1) and pk[1] == -3.0 and np.array_equal(s[1], np.float32([-1, 0, 1])), "NaN neighbours: delta is 0"


def test_parabola_is_fitted_and_guarded_per_axis():
    c = np.zeros((1, 5, 6, 7), dtype=np.float32)
    c[0, 1, 2, 3] = 2.0
    c[0, 0, 2, 3], c[0, 2, 2, 3] = 1.0, 1.5                                # z: a proper parabola
    c[0, 1, 1, 3], c[0, 1, 3, 3] = 0.5, 2.0                                # y: clamped to +0.5 (a plateau with the upper neighbour)
    c[0, 1, 2, 2], c[0, 1, 2, 4] = np.nan, 1.0                             # x: a NaN neighbour, no refinement
    s, ip, pk = R3.peak(c, (2, 2, 3))
    assert tuple(ip[0]) == (1, 2, 3) and pk[0] == 2.0
    want = (1.0 + R.delta(1.0, 2.0, 1.5), 2.0 + R.delta(0.5, 2.0, 2.0), 3.0)
    assert R.delta(0.5, 2.0, 2.0) == 0.5 and 0.0 < R.delta(1.0, 2.0, 1.5) < 0.5
    assert np.array_equal(s[0], np.float32(want))
    assert np.array_equal(R3.peak(c, (2, 2, 3), subpixel=False)[0][0], np.float32([1, 2, 3]))
    c1 = np.zeros((1, 1, 6, 7), dtype=np.float32)                          # D = 1: the z neighbours are the peak itself, den = 0
    c1[0, 0, 2, 3], c1[0, 0, 2, 4] = 2.0, 1.0
    assert R3.peak(c1, (0, 2, 3))[0][0, 0] == 0.0


def test_zero_weight_plane_does_not_propagate_a_nan_plane():
    x = np.arange(3 * 4 * 5, dtype=np.float32).reshape(1, 3, 4, 5)
    x[0, 1] = np.nan
    x[0, 2, 1, 1], x[0, 0, 0, 0] = np.inf, -0.0
    out = R3.shift(x, np.float32([[2.0, 1.0, -2.0]]), fill=-7.0)           # plane 0 <- plane 2, planes 1 and 2 from outside
    want = np.full((3, 4, 5), -7.0, dtype=np.float32)
    want[0, 0:3, 2:5] = x[0, 2, 1:4, 0:3]
    assert np.array_equal(u32(out[0]), u32(want)), "an integer shift copies bits and never reads the NaN plane"
    assert u32(R3.shift(x, np.float32([[0.0, 0.0, 0.0]]))[0])[0, 0, 0] == 0x80000000, "-0 survives"
    half = R3.shift(x, np.float32([[0.5, 0.0, 0.0]]), fill=1.0)[0]
    assert np.isnan(half[0]).all() and np.isnan(half[1]).all(), "a half step blends the NaN plane in"
    assert np.array_equal(half[2, 0], np.float32(0.5) * x[0, 2, 0] + np.float32(0.5)), "and the fill plane behind the volume"
    tiny = R3.shift(x, np.float32([[-1e-10, 0.0, 0.0]]), fill=9.0)[0]     # fl(dz - floor(dz)) == 1: weights (0, 1), plane z itself
    assert np.array_equal(u32(tiny), u32(x[0])), "the plane of weight 0 (z - 1, outside the volume for z = 0) is not added"
    for bad in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]):
        assert np.array_equal(R3.shift(x, np.float32([bad]), fill=3.0)[0], np.full((3, 4, 5), 3.0, np.float32))
    for far in (3.0, -3.0, 1e30, -1e30):
        assert np.array_equal(R3.shift(x, np.float32([[far, 0, 0]]), fill=3.0)[0], np.full((3, 4, 5), 3.0, np.float32)), "|dz| >= D"


@pytest.mark.parametrize("d,want", [(0.5, 0), (-0.5, 0), (1.5, 2), (-1.5, -2), (2.5, 2), (0.75, 1)])
def test_nearest_is_rintf_on_every_axis(d, want):
    x = (np.arange(6 * 6 * 6, dtype=np.float32) + 1).reshape(1, 6, 6, 6)
    for axis in range(3):
        s = np.zeros((1, 3), dtype=np.float32)
        s[0, axis] = d
        out = R3.shift(x, s, mode="nearest")[0]
        ref = np.zeros((6, 6, 6), dtype=np.float32)
        src = [slice(max(0, want), 6 + min(0, want))] * 3
        dst = [slice(max(0, -want), 6 - max(0, want))] * 3
        sel_s, sel_d = [slice(None)] * 3, [slice(None)] * 3
        sel_s[axis], sel_d[axis] = src[axis], dst[axis]
        ref[tuple(sel_d)] = x[0][tuple(sel_s)]
        assert np.array_equal(out, ref), (axis, d)


def test_depth_one_is_the_two_dimensional_restatement_bit_for_bit():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3, 1, 9, 13)).astype(np.float32)
    x[1, 0, 4, 5], x[2, 0, 0, 0] = np.nan, -0.0
    wy, wx = R.taper_window(9, 2), R.taper_window(13, 3)
    assert np.array_equal(u32(R3.window(x, np.ones(1, np.float32), wy, wx)[:, 0]), u32(R.window(x[:, 0], wy, wx)))
    c = rng.standard_normal((4, 1, 9, 13)).astype(np.float32)
    c[3, 0] = np.nan
    for sub in (True, False):
        s3, i3, p3 = R3.peak(c, (0, 3, 5), sub)
        s2, i2, p2 = R.peak(c[:, 0], (3, 5), sub)
        assert np.array_equal(u32(s3[:, 1:]), u32(s2)) and np.array_equal(i3[:, 1:], i2) and np.array_equal(u32(p3), u32(p2))
        assert not s3[:, 0].any() and not i3[:, 0].any()
    sh = np.float32([[0.0, 1.25, -2.5], [0.0, -0.75, 3.0], [0.0, 2.0, 0.0]])
    for mode in ("bilinear", "nearest"):
        assert np.array_equal(u32(R3.shift(x, sh, mode, fill=-1.5)[:, 0]), u32(R.shift(x[:, 0], sh[:, 1:], mode, fill=-1.5)))


# ------------------------------------------------------------------------------------------------ the planted scene
@pytest.mark.parametrize("shape,max_d,taper", CASES)
def test_planted_integer_displacements_are_recovered_exactly(shape, max_d, taper):
    worst = 0.0
    m = tuple(v + 1 for v in max_d)
    for seed in SEEDS:
        sc = R3.scene(seed, *shape, max_d=max_d)
        assert sc.volumes.shape == (6,) + shape
        c = R3.correlate(sc.volumes, sc.template, taper)
        s, ip, pk = R3.peak(c, m, subpixel=False)
        assert np.array_equal(ip, sc.shifts.astype(np.int32)) and np.array_equal(s, sc.shifts), (shape, seed)
        for n in range(c.shape[0]):
            mm = c[n].copy()
            for a in (-1, 0, 1):
                for b in (-1, 0, 1):
                    for e in (-1, 0, 1):
                        mm[(ip[n, 0] + a) % shape[0], (ip[n, 1] + b) % shape[1], (ip[n, 2] + e) % shape[2]] = -np.inf
            ratio = float(mm.max() / pk[n])
            worst = max(worst, ratio)
            assert ratio <= CAP, f"{shape}, seed {seed}, volume {n}: second peak / peak = {ratio:.3f}"
        if seed < 2:
            reg = R3.shift(sc.volumes, s, mode="nearest")
            z0, z1, y0, y1, x0, x1 = R3.valid_box(s, shape)
            assert np.array_equal(u32(reg[:, z0:z1, y0:y1, x0:x1]), u32(sc.still[:, z0:z1, y0:y1, x0:x1])), "an exact crop of the still scene"
    print(f"{shape}: largest second peak / peak = {worst:.3f} (measured 0.404 and 0.174)")


@pytest.mark.parametrize("shape,max_d,taper", CASES)
def test_planted_subvoxel_displacements(shape, max_d, taper):
    worst = 0.0
    m = tuple(v + 1 for v in max_d)
    for seed in SEEDS:
        sc = R3.scene(seed, *shape, max_d=max_d, subpixel=True)
        s, ip, _ = R3.peak(R3.correlate(sc.volumes, sc.template, taper), m)
        assert np.all(np.abs(ip - sc.shifts) < 1.0), (shape, seed)       # the floor or the ceiling: near a half either is right
        worst = max(worst, float(np.abs(s - sc.shifts).max()))
    print(f"{shape}: worst sub-voxel error {worst:.4f} voxels (measured 0.361 and 0.267)")
    assert worst <= SUBVOXEL_BOUND


def test_valid_box_is_the_box_every_registered_volume_covers():
    from cwfa_amd.CWFA import valid_box
    assert valid_box(torch.zeros(3, 3), (6, 10, 12)) == (0, 6, 0, 10, 0, 12)
    assert valid_box(torch.zeros(0, 3), (6, 10, 12)) == (0, 6, 0, 10, 0, 12)
    assert valid_box(torch.tensor([[1.0, 2.0, -3.0], [-2.0, -1.0, 1.0]]), (6, 10, 12)) == (2, 5, 1, 8, 3, 11)
    assert valid_box(torch.tensor([[0.5, 0.25, -0.25]]), (6, 10, 12)) == (0, 5, 0, 9, 1, 12), "a fractional shift reads one voxel further"
    assert valid_box(torch.tensor([[0.0, float("nan"), 0.0]]), (6, 10, 12)) == (0,) * 6
    assert valid_box(torch.tensor([[6.0, 0.0, 0.0]]), (6, 10, 12)) == (0,) * 6
    assert valid_box(torch.tensor([[3.0, 0.0, 0.0], [-3.0, 0.0, 0.0]]), (6, 10, 12)) == (0,) * 6, "nothing is left"
    with pytest.raises(ValueError, match="shape"):
        valid_box(torch.zeros(1, 3), (10, 12))
    for seed in range(4):
        s = np.random.default_rng(seed).uniform(-3, 3, size=(6, 3)).astype(np.float32)
        assert valid_box(torch.from_numpy(s), (8, 20, 30)) == R3.valid_box(s, (8, 20, 30))


# ------------------------------------------------------------------------------------------------ the entry points' arguments
def test_reg_window3d_arguments(L, ptr):
    x, wz, wy, wx, out = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(5))

    def call(x=x, N=2, D=3, H=4, W=8, vs=96, wz=wz, wy=wy, wx=wx, out=out):
        return L.cwfa_reg_window3d_f32(x, N, D, H, W, vs, wz, wy, wx, out, None)

    for k in ("x", "wz", "wy", "wx", "out"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_window3d_f32: null" in L.cwfa_last_error()
    assert call(N=-1) == -2 and call(D=-3) == -2 and call(H=-4) == -2 and call(W=-8) == -2 and b"negative" in L.cwfa_last_error()
    assert call(D=1 << 10, H=1 << 11, W=1 << 10) == -2 and call(D=1 << 30) == -2 and b"too large" in L.cwfa_last_error()
    for k in ("x", "wz", "wy", "wx", "out"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 8192 + 2)}) == -3 and b"4-byte" in L.cwfa_last_error(), k
    assert call(vs=95) == -1 and call(vs=-96) == -1 and b"stride" in L.cwfa_last_error()
    assert call(out=x) == -1 and b"must not" in L.cwfa_last_error()
    assert call(N=0) == 0 and call(D=0, vs=0) == 0 and call(H=0, vs=0) == 0 and call(W=0, vs=0) == 0, "empty: no launch"


def test_reg_peak3d_arguments(L, ptr):
    c, shifts, ipeak, peak = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(4))

    def call(c=c, N=2, D=3, H=5, W=9, vs=135, mz=1, my=2, mx=4, sub=1, shifts=shifts, ipeak=ipeak, peak=peak):
        return L.cwfa_reg_peak3d_f32(c, N, D, H, W, vs, mz, my, mx, sub, shifts, ipeak, peak, None)

    for k in ("c", "shifts", "ipeak", "peak"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_peak3d_f32: null" in L.cwfa_last_error()
    assert call(sub=2) == -1 and call(sub=-1) == -1 and b"subpixel" in L.cwfa_last_error()
    for k in ("N", "D", "H", "W", "mz", "my", "mx"):
        assert call(**{k: -1}) == -2 and b"negative" in L.cwfa_last_error(), k
    assert call(D=1 << 10, H=1 << 11, W=1 << 10) == -2 and b"too large" in L.cwfa_last_error()
    assert call(mz=2) == -2 and call(my=3) == -2 and call(mx=5) == -2 and b"wider than" in L.cwfa_last_error(), "2 m + 1 <= the side"
    assert call(mz=1 << 30) == -2 and call(mx=(1 << 31) - 1) == -2, "no overflow in 2 m + 1"
    assert call(vs=134) == -1 and b"stride" in L.cwfa_last_error()
    for k in ("c", "shifts", "ipeak", "peak"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 8192 + 2)}) == -3 and b"4-byte" in L.cwfa_last_error(), k
    assert call(N=0) == 0 and call(D=0, vs=0, mz=0) == 0 and call(H=0, vs=0, my=0) == 0 and call(W=0, vs=0, mx=0) == 0, "empty: no launch"


def test_reg_shift3d_arguments(L, ptr):
    x, shifts, out = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(3))

    def call(x=x, N=2, D=3, H=4, W=8, vs=96, shifts=shifts, mode=0, fill=0.0, out=out):
        return L.cwfa_reg_shift3d_f32(x, N, D, H, W, vs, shifts, mode, fill, out, None)

    for k in ("x", "shifts", "out"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_shift3d_f32: null" in L.cwfa_last_error()
    assert call(mode=2) == -1 and call(mode=-1) == -1 and b"mode" in L.cwfa_last_error()
    assert call(N=-1) == -2 and call(D=-1) == -2 and call(H=-1) == -2 and call(W=-1) == -2 and b"negative" in L.cwfa_last_error()
    assert call(D=1 << 10, H=1 << 11, W=1 << 10) == -2 and call(W=1 << 30, D=1, H=1) == -2 and b"too large" in L.cwfa_last_error()
    for k in ("x", "shifts", "out"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 8192 + 2)}) == -3 and b"4-byte" in L.cwfa_last_error(), k
    assert call(vs=95) == -1 and call(vs=-97) == -1 and b"stride" in L.cwfa_last_error(), "a stride that volumes overlap under"
    assert call(out=x) == -1 and b"alias" in L.cwfa_last_error()
    assert call(N=0) == 0 and call(D=0, vs=0) == 0 and call(H=0, vs=0) == 0 and call(W=0, vs=0) == 0, "empty: no launch"


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_python_layer_refuses_before_any_device_work():
    from cwfa_amd import ops
    from cwfa_amd.CWFA import estimate_volume_shifts, register_volumes, shift_volumes
    v = torch.zeros(4, 6, 40, 48)
    t = torch.zeros(6, 40, 48)
    sh = torch.zeros(4, 3)
    for call in (lambda: estimate_volume_shifts(v[..., ::2], t[..., ::2]), lambda: register_volumes(v[:, :, ::2]), lambda: shift_volumes(v[..., ::2], sh),
                 lambda: estimate_volume_shifts(v[0], t), lambda: register_volumes(v[0]), lambda: shift_volumes(v[0], sh)):
        with pytest.raises(ValueError, match=r"contiguous \[N,D,H,W\]"):
            call()
    for call in (lambda: estimate_volume_shifts(v.half(), t), lambda: register_volumes(v.double(), t), lambda: shift_volumes(v.half(), sh)):
        with pytest.raises(ValueError, match="float32 stack"):
            call()
    for bad in (torch.zeros(6, 40, 47), torch.zeros(1, 6, 40, 48), torch.zeros(6, 40, 48, dtype=torch.float64)):
        with pytest.raises(ValueError, match="template"):
            estimate_volume_shifts(v, bad)
        with pytest.raises(ValueError, match="template"):
            register_volumes(v, bad)
    with pytest.raises(ValueError, match="template"):
        estimate_volume_shifts(v, None)
    for fn in (estimate_volume_shifts, register_volumes):
        with pytest.raises(ValueError, match="'dft'.*not built"):
            fn(v, t, subpixel="dft")
        with pytest.raises(ValueError, match="subpixel"):
            fn(v, t, subpixel="parabola")
    for out in (v, v[:], v[1:]):
        with pytest.raises(ValueError, match="alias"):
            shift_volumes(v, sh, out=out)
    with pytest.raises(ValueError, match="alias"):
        register_volumes(v, t, out=v)
    for n_iter in (0, -1):
        with pytest.raises(ValueError, match="n_iter"):
            register_volumes(v, t, n_iter=n_iter)
    for m in (20, (3, 8, 8), (2, 20, 8), (2, 8, 24), (1, -1, 1), (2, 8), "x"):
        with pytest.raises(ValueError, match="max_shift"):
            estimate_volume_shifts(v, t, max_shift=m)
    for tp in (4, (4, 0, 0), (0, 21, 0), (0, 0, -1), (1, 1)):
        with pytest.raises(ValueError, match="taper"):
            estimate_volume_shifts(v, t, taper=tp)
    with pytest.raises(ValueError, match="chunk"):
        estimate_volume_shifts(v, t, chunk=0)
    with pytest.raises(ValueError, match="smooth and eps"):
        estimate_volume_shifts(v, t, smooth=-1.0)
    with pytest.raises(ValueError, match="mode"):
        shift_volumes(v, sh, mode="cubic")
    with pytest.raises(ValueError, match="mode"):
        register_volumes(v, t, mode="cubic")
    for bad in (torch.zeros(3, 3), torch.zeros(4, 2), torch.zeros(4, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="shifts"):
            shift_volumes(v, bad)
    with pytest.raises(ValueError, match="max_shift"):
        ops._max_shift3((1, 2, 25), 6, 40, 48, "reg_peak3d")
    assert ops._max_shift3(2, 6, 40, 48, "t") == (2, 2, 2) and ops._max_shift3((2, 19, 23), 6, 40, 48, "t") == (2, 19, 23), "2 m + 1 == the side"
    for call in (lambda: estimate_volume_shifts(v, t), lambda: shift_volumes(v, sh), lambda: register_volumes(v, t),
                 lambda: ops.reg_window3d(v, t[:, 0, 0], t[0, :, 0], t[0, 0]), lambda: ops.reg_peak3d(v, 2), lambda: ops.reg_shift3d(v, sh)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_the_names_are_exported_next_to_the_activity_map():
    from cwfa_amd import CWFA
    for name in ("estimate_volume_shifts", "shift_volumes", "register_volumes", "VolumeRegistration", "VolumeRegistrar", "valid_box"):
        assert name in CWFA.__all__ and hasattr(CWFA, name)
    assert CWFA.VolumeRegistration._fields == ("volumes", "shifts", "peak", "template")
    assert "fp.update(reg(inverse_pass(" in CWFA.VolumeRegistrar.__doc__ and "find_neurons" in CWFA.valid_box.__doc__
