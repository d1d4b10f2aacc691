"""GPU: rigid registration of volumes.  The three kernels bit for bit against the numpy restatement
tests/register3d_ref.py on the SAME inputs -- correlation maps are handed in, so no FFT difference enters -- at the smallest shapes
that reach every path (one voxel, odd sizes on the element path, the 16-byte path, a volume stride, a base that breaks 16-byte
alignment, more planes than one z segment of the resampling, more volumes than a grid axis holds); the D = 1 forms against the 2-D
kernels; then ``register_volumes`` end to end on the planted scene, where an integer displacement is recovered exactly and undone
bit for bit, which makes the ``ActivityMap`` of the registered series the ``ActivityMap`` of the still scene."""
import functools

import numpy as np
import pytest
import torch

import register3d_ref as R3
import register_ref as R
from test_gpu_register import device_stack, same_bits, same_values

pytestmark = pytest.mark.gpu

# (N, D, H, W, unused elements behind every volume, elements in front of the first volume).  12 x 16: the 16-byte forms; 10 x 13:
# element by element; 17 and 33 planes: two and three z segments of the resampling (a segment holds at most 16)
LAYOUTS = [(1, 1, 1, 1, 0, 0), (3, 2, 5, 7, 0, 0), (2, 5, 12, 16, 0, 0), (2, 6, 10, 13, 0, 0), (2, 5, 12, 16, 8, 0), (2, 5, 12, 16, 3, 0),
           (2, 5, 12, 16, 0, 1), (2, 2, 5, 7, 2, 3), (1, 17, 4, 8, 0, 0), (2, 33, 3, 5, 1, 0)]
CASES = (((12, 24, 28), (2, 3, 3), (1, 3, 3)), ((16, 37, 45), (3, 4, 4), (2, 4, 4)))
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def volume_data(N, D, H, W, specials=True):
    rng = np.random.default_rng(23 + 1000 * N + 100 * D + 10 * H + W)
    x = (rng.standard_normal((N, D, H, W)) * 100.0 + 300.0).astype(np.float32)
    if specials and H >= 3 and W >= 4:
        z = min(1, D - 1)
        x[0, 0, 1, 2], x[0, z, 2, 3], x[N - 1, D - 1, H - 1, W - 1], x[0, 0, 0, 0], x[0, z, H - 1, 1] = np.nan, np.inf, -np.inf, -0.0, 0.0
    return x


# ------------------------------------------------------------------------------------------------ the window
@pytest.mark.parametrize("N,D,H,W,pad,offset", LAYOUTS)
def test_window_bit_for_bit(N, D, H, W, pad, offset):
    from cwfa_amd import ops
    x = volume_data(N, D, H, W, specials=False)
    wz, wy, wx = R.taper_window(D, min(2, D // 2)), R.taper_window(H, min(4, H // 2)), R.taper_window(W, min(4, W // 2))
    want = R3.window(x, wz, wy, wx)
    got = ops.reg_window3d(device_stack(x, pad, offset), dev(wz), dev(wy), dev(wx))
    assert got.dtype == torch.float32 and same_bits(got, want)
    out = torch.empty(N, D, H, W, device="cuda")
    assert ops.reg_window3d(device_stack(x, pad, offset), dev(wz), dev(wy), dev(wx), out=out) is out and same_bits(out, want)
    ones = ops.reg_window3d(device_stack(x, pad, offset), torch.ones(D, device="cuda"), torch.ones(H, device="cuda"), torch.ones(W, device="cuda"))
    assert same_bits(ones, x), "taper 0: the stack itself"


def test_window_with_an_unaligned_window_vector():
    from cwfa_amd import ops
    x = volume_data(2, 3, 8, 16, specials=False)
    wz, wy, wx = R.taper_window(3, 1), R.taper_window(8, 3), R.taper_window(16, 5)
    wxd = device_stack(wx[None], 0, 1, gap=9.0)[0]                          # wx at a 4-byte offset: the element path
    assert same_bits(ops.reg_window3d(dev(x), dev(wz), dev(wy), wxd), R3.window(x, wz, wy, wx))


def test_more_volumes_than_a_grid_axis_holds():
    """N = 70 000 volumes of 1 x 1 x 4: the kernels walk the volumes, no grid axis grows with N."""
    from cwfa_amd import ops
    N = 70000
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, 1, 1, 4)).astype(np.float32)
    xd = dev(x)
    wx = np.float32([0.25, 1.0, 1.0, 0.5])
    got = ops.reg_window3d(xd, torch.ones(1, device="cuda"), torch.ones(1, device="cuda"), dev(wx))
    assert same_bits(got, x * wx[None, None, None, :])
    s, i, p = ops.reg_peak3d(xd, (0, 0, 1), subpixel=False)                 # the window reads x = 3, 0, 1: shifts -1, 0, 1
    win = x[:, 0, 0, [3, 0, 1]]
    wi = np.argmax(win, axis=1)                                             # the first maximum: the lowest index
    want_i = np.stack([np.zeros(N), np.zeros(N), wi - 1], axis=1).astype(np.int32)
    assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(s.cpu().numpy(), want_i.astype(np.float32))
    assert same_bits(p, win[np.arange(N), wi])
    d = np.zeros((N, 3), dtype=np.float32)
    d[:, 2] = rng.integers(-1, 2, size=N)
    d[N - 1] = (0.0, 0.0, 0.5)
    got = ops.reg_shift3d(xd, dev(d), fill=-2.0).cpu().numpy()
    want = np.full((N, 4), -2.0, dtype=np.float32)
    row = x[:, 0, 0]
    for k in (-1, 0, 1):
        sel = d[:, 2] == k
        lo, hi = max(0, -k), min(4, 4 - k)
        want[sel, lo:hi] = row[sel, lo + k:hi + k]
    want[N - 1] = R3.shift(x[N - 1:], d[N - 1:], fill=-2.0)[0, 0, 0]
    assert same_bits(got[:, 0, 0], want), "every volume, the last one included"


# ------------------------------------------------------------------------------------------------ the peak
def corr_maps(N, D, H, W, kind, m):
    mz, my, mx = m
    rng = np.random.default_rng(3 + 1000 * N + 100 * D + 10 * H + W + 49 * mz + 7 * my + mx)
    c = (0.05 * rng.standard_normal((N, D, H, W))).astype(np.float32)
    big = np.float32(0.8)
    for n in range(N):
        if kind == "random":
            continue
        if kind == "wrap":                                                  # negative shifts: the far side of the map, axis by axis
            s = [0, 0, 0]
            s[n % 3] = -min(m[n % 3], 1 + n % 2)
            if n >= 3:
                s = [-min(mz, 1), -min(my, 2), -min(mx, 1)]
        elif kind == "border":                                              # on the window's border: a parabola neighbour lies outside
            s = (mz, my, -mx) if n % 2 == 0 else (-mz, -my, mx)
        else:
            s = (0, 0, 0)
        z, y, x = s[0] % D, s[1] % H, s[2] % W
        if kind == "plateau":
            c[n] = np.float32(0.25)
            if D * H * W > 1 and n % 2:
                c[n, 0, 0, 0] = -0.0
        elif kind == "specials":
            c[n] = rng.choice(np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.3, -0.7, 0.3]), size=(D, H, W),
                              p=[0.3, 0.02 * (n % 2), 0.1, 0.15, 0.15, 0.1, 0.08 + 0.02 * (1 - n % 2), 0.1])
        elif kind == "nan":
            c[n] = np.nan
            if n % 2 and H > 2 * my + 1:
                c[n, 0, (my + 1) % H, 0] = -np.inf                          # outside the window
        else:
            c[n, z, y, x] = big
            c[n, (z + 1) % D, y, x] += np.float32(0.2)                       # uneven neighbours: a delta away from 0 on every axis
            c[n, z, (y + 1) % H, x] += np.float32(0.3)
            c[n, z, y, (x - 1) % W] += np.float32(0.45)
    return c


PEAK_SHAPES = [(1, 1, 1, 1, 0, 0), (4, 3, 5, 7, 0, 0), (4, 5, 12, 16, 0, 0), (4, 6, 10, 13, 5, 0), (3, 5, 12, 16, 0, 1)]


@pytest.mark.parametrize("kind", ["random", "wrap", "border", "plateau", "specials", "nan"])
@pytest.mark.parametrize("N,D,H,W,pad,offset", PEAK_SHAPES)
def test_peak_bit_for_bit(N, D, H, W, pad, offset, kind):
    from cwfa_amd import ops
    full = ((D - 1) // 2, (H - 1) // 2, (W - 1) // 2)                       # odd sides: 2 m + 1 == the side on that axis
    windows = {(0, 0, 0), (min(1, full[0]), min(2, full[1]), min(3, full[2])), full, (0, full[1], min(3, full[2])), (full[0], 0, 0)}
    for m in sorted(windows):
        c = corr_maps(N, D, H, W, kind, m)
        cd = device_stack(c, pad, offset, gap=9.0)
        for sub in (True, False):
            ws, wi, wp = R3.peak(c, m, sub)
            s, i, p = ops.reg_peak3d(cd, m, sub)
            what = f"{kind} {N}x{D}x{H}x{W} window {m} subpixel {sub}"
            assert np.array_equal(i.cpu().numpy(), wi), what
            assert same_bits(s, ws) and same_bits(p, wp), what
            if not sub:
                assert np.array_equal(s.cpu().numpy(), wi.astype(np.float32)), "the integer peak as fp32"
        assert all(same_bits(a, b) for a, b in zip(ops.reg_peak3d(cd, m, True), ops.reg_peak3d(cd, m, True))), "two runs, bitwise"
    if kind in ("wrap", "border") and min(D, H, W) >= 3:
        m = (min(1, full[0]), min(2, full[1]), min(3, full[2]))
        ws, wi, _ = R3.peak(corr_maps(N, D, H, W, kind, m), m, True)
        assert (wi < 0).any(axis=0).all(), "a maximum on the wrap side of every axis"
        if kind == "border":
            assert np.all(np.abs(wi) == np.array(m)) and np.any(ws != wi), "on the border, refined from outside the window"


def test_peak_accepts_an_int_and_writes_into_out():
    from cwfa_amd import ops
    c = corr_maps(4, 7, 16, 24, "wrap", (3, 3, 3))
    out = (torch.empty(6, 3, device="cuda")[1:5], torch.empty(6, 3, dtype=torch.int32, device="cuda")[1:5], torch.empty(6, device="cuda")[1:5])
    got = ops.reg_peak3d(dev(c), 3, out=out)
    assert all(a is b for a, b in zip(got, out))
    assert all(same_bits(a, b) for a, b in zip(got, R3.peak(c, 3)))


# ------------------------------------------------------------------------------------------------ D = 1: the 2-D kernels
@pytest.mark.parametrize("N,H,W,pad,offset", [(1, 1, 1, 0, 0), (3, 5, 7, 0, 0), (2, 12, 16, 0, 0), (2, 12, 16, 4, 0), (3, 10, 13, 2, 1)])
def test_depth_one_is_the_two_dimensional_kernel_bit_for_bit(N, H, W, pad, offset):
    """The window is one kernel for frames and volumes, so the window part here compares that kernel with itself through its two
    entry points (each entry point is held against its own restatement in ``test_window_bit_for_bit`` of this file and of
    test_gpu_register.py).  The peak and the resampling parts still compare two kernels."""
    from cwfa_amd import ops
    x = volume_data(N, 1, H, W)
    xd = device_stack(x, pad, offset)
    wy, wx = dev(R.taper_window(H, min(3, H // 2))), dev(R.taper_window(W, min(4, W // 2)))
    assert same_bits(ops.reg_window3d(xd, torch.ones(1, device="cuda"), wy, wx)[:, 0], ops.reg_window(xd[:, 0], wy, wx))
    my, mx = min(2, (H - 1) // 2), min(3, (W - 1) // 2)
    c = corr_maps(N, 1, H, W, "wrap", (0, my, mx))
    c[N - 1] = np.nan
    cd = device_stack(c, pad, offset, gap=9.0)
    for sub in (True, False):
        s3, i3, p3 = ops.reg_peak3d(cd, (0, my, mx), sub)
        s2, i2, p2 = ops.reg_peak(cd[:, 0], (my, mx), sub)
        assert same_bits(s3[:, 1:], s2) and same_bits(i3[:, 1:], i2) and same_bits(p3, p2)
        assert not bool(s3[:, 0].any()) and not bool(i3[:, 0].any())
    table = np.float32([[0.0, 1.25, -2.5], [0.0, -0.75, 3.0], [-0.0, 2.0, 0.0], [0.0, 0.5, 0.5], [0.0, np.nan, 1.0]])
    for k in range(0, len(table), N):
        d = np.resize(table[k:k + N], (N, 3)).astype(np.float32)
        for mode in ("bilinear", "nearest"):
            got = ops.reg_shift3d(xd, dev(d), mode=mode, fill=-1.5)
            assert same_bits(got[:, 0], ops.reg_shift(xd[:, 0], dev(d[:, 1:]), mode=mode, fill=-1.5)), (d.tolist(), mode)


# ------------------------------------------------------------------------------------------------ the resampling
def integer_shift_reference(x, d, fill):
    out = np.full(x.shape, fill, dtype=x.dtype)
    for n in range(x.shape[0]):
        src, dst = [], []
        for a, side in enumerate(x.shape[1:]):
            k = int(d[n][a])
            lo, hi = max(0, -k), min(side, side - k)
            src.append(slice(lo + k, max(hi + k, lo + k)))
            dst.append(slice(lo, max(hi, lo)))
        out[n][tuple(dst)] = x[n][tuple(src)]
    return out


@pytest.mark.parametrize("N,D,H,W,pad,offset", LAYOUTS)
def test_integer_shifts_copy_bits(N, D, H, W, pad, offset):
    from cwfa_amd import ops
    x = volume_data(N, D, H, W)
    rng = np.random.default_rng(N + D + H + W)
    lim = np.array([min(2, D), min(3, H), min(3, W)])
    d = rng.integers(-lim, lim + 1, size=(N, 3)).astype(np.float32)
    d[0] = 0
    d[N - 1] = (-0.0, 0.0, 1.0 if W > 1 else 0.0)
    xd = device_stack(x, pad, offset)
    for fill in (0.0, -7.5):
        want = integer_shift_reference(x, d, fill)
        for mode in ("bilinear", "nearest"):
            got = ops.reg_shift3d(xd, dev(d), mode=mode, fill=fill)
            assert got.dtype == torch.float32 and same_bits(got, want), (mode, fill)
        assert same_bits(R3.shift(x, d, "bilinear", fill), want), "the restatement agrees"
    near = d + np.float32(0.25) * np.float32(rng.choice([-1, 1], size=d.shape))
    assert same_bits(ops.reg_shift3d(xd, dev(near), mode="nearest", fill=-7.5), integer_shift_reference(x, d, -7.5))


@pytest.mark.parametrize("N,D,H,W,pad,offset", LAYOUTS)
def test_integer_dz_gives_the_two_dimensional_resampling_of_the_moved_plane(N, D, H, W, pad, offset):
    from cwfa_amd import ops
    x = volume_data(N, D, H, W)
    xd = device_stack(x, pad, offset)
    table = np.float32([[1.0, 0.5, -0.25], [-1.0, -1.75, 2.3], [0.0, 0.3, 0.0], [2.0, -0.001, 0.999], [-3.0, 0.5, 0.5], [float(D), 0.25, 0.25]])
    for k in range(0, len(table), N):
        d = np.resize(table[k:k + N], (N, 3)).astype(np.float32)
        for fill in (0.0, 2.5):
            got = ops.reg_shift3d(xd, dev(d), fill=fill)
            for n in range(N):
                planes = ops.reg_shift(xd[n], dev(np.tile(d[n:n + 1, 1:], (D, 1))), fill=fill)      # every plane of the volume under (dy, dx)
                want = torch.full_like(planes, fill)
                k0 = int(d[n, 0])
                lo, hi = max(0, -k0), min(D, D - k0)
                if hi > lo:
                    want[lo:hi] = planes[lo + k0:hi + k0]
                assert same_bits(got[n], want), (d[n].tolist(), fill)


@pytest.mark.parametrize("N,D,H,W,pad,offset", LAYOUTS)
def test_fractional_shifts_bit_for_bit(N, D, H, W, pad, offset):
    from cwfa_amd import ops
    x = volume_data(N, D, H, W)
    xd = device_stack(x, pad, offset)
    table = np.float32([[0.5, 0.5, 0.5], [-0.5, 1.5, -0.5], [0.25, 0.0, 0.0], [-1.75, 0.0, 0.25], [1.3, 2.3, -3.6], [-0.001, -0.001, 0.999],
                        [float(D), 0.4, 0.0], [-float(D) - 0.5, 0.0, 0.3], [float(D) - 0.5, 0.0, 0.0], [0.3, float(H), -float(W) - 2.5],
                        [np.nan, 0.0, 0.0], [0.5, np.inf, 0.0], [0.5, 0.5, np.nan], [1e30, 0.0, 0.0], [-1e30, 0.5, 0.5], [0.5, 1e30, -1e30],
                        [-1e-10, 0.0, 0.0], [1e-30, 1e-30, 1e-30], [0.5, 1.0, -2.0], [3e9, 0.5, 0.5]])
    for k in range(0, len(table), max(N, 1)):
        d = np.resize(table[k:k + N], (N, 3)).astype(np.float32)
        for mode in ("bilinear", "nearest"):
            for fill in (0.0, 2.5):
                want = R3.shift(x, d, mode, fill)
                got = ops.reg_shift3d(xd, dev(d), mode=mode, fill=fill)
                assert got.dtype == torch.float32 and same_values(got, want), (d.tolist(), mode, fill)
    out = torch.empty(N, D, H, W, device="cuda")
    d = np.resize(table[:N], (N, 3)).astype(np.float32)
    assert ops.reg_shift3d(xd, dev(d), out=out) is out and same_values(out, R3.shift(x, d))


def test_ops_refuse_aliasing_and_bad_arguments():
    from cwfa_amd import ops
    x = torch.zeros(2, 4, 8, 8, device="cuda")
    s = torch.zeros(2, 3, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        ops.reg_shift3d(x, s, out=x)
    with pytest.raises(ValueError, match="alias"):
        ops.reg_window3d(x, x[0, :, 0, 0], x[0, 0, 0], x[0, 0, 0], out=x)
    with pytest.raises(ValueError, match="mode"):
        ops.reg_shift3d(x, s, mode="cubic")
    with pytest.raises(ValueError, match="max_shift"):
        ops.reg_peak3d(x, (2, 3, 3))
    with pytest.raises(ValueError, match="shifts"):
        ops.reg_shift3d(x, s[:1])
    with pytest.raises(TypeError, match="float32"):
        ops.reg_shift3d(x.half(), s)
    with pytest.raises(ValueError, match=r"\[N, D, H, W\]"):
        ops.reg_peak3d(x[0], 1)


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def planted(seed, shape=CASES[0][0], max_d=CASES[0][1], subpixel=False, rest=0):
    return R3.scene(seed, *shape, max_d=max_d, subpixel=subpixel, rest=rest)


KW = dict(max_shift=(3, 4, 4), taper=(1, 3, 3))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_integer_displacements_are_undone_bit_for_bit(seed):
    from cwfa_amd.CWFA import ActivityMap, VolumeRegistrar, register_volumes, valid_box
    sc = planted(seed)
    shape = sc.volumes.shape[1:]
    volumes, still, template = dev(sc.volumes), dev(sc.still), dev(sc.template)
    reg = register_volumes(volumes, template, subpixel=False, mode="nearest", **KW)
    assert np.array_equal(reg.shifts.cpu().numpy(), sc.shifts), "exactly the planted displacements"
    assert reg.template is template and reg.volumes.dtype == torch.float32 and tuple(reg.peak.shape) == (6,) and tuple(reg.shifts.shape) == (6, 3)
    z0, z1, y0, y1, x0, x1 = box = valid_box(reg.shifts, shape)
    assert box == R3.valid_box(sc.shifts, shape) and z1 - z0 >= shape[0] - 4 and y1 - y0 >= shape[1] - 6 and x1 - x0 >= shape[2] - 6
    crop = lambda t: t[..., z0:z1, y0:y1, x0:x1].contiguous()
    assert same_bits(crop(reg.volumes), sc.still[:, z0:z1, y0:y1, x0:x1]), "the registered stack is the still scene"
    assert same_bits(register_volumes(volumes, template, subpixel=False, **KW).volumes, reg.volumes), "an integer shift: trilinear copies bits too"
    assert same_bits(register_volumes(volumes, template, subpixel=False, mode="nearest", chunk=4, **KW).shifts, reg.shifts), "any chunking"

    registrar = VolumeRegistrar(template, mode="nearest", subpixel=False, **KW)
    a, b, moved = (ActivityMap(shape, "cuda") for _ in range(3))
    for s, e in ((0, 4), (4, 6)):                                           # the series in two chunks, never resident
        a.update(registrar(volumes[s:e]))
    assert len(registrar.shifts) == 2 and same_bits(registrar.all_shifts(), reg.shifts) and same_bits(registrar.all_peaks(), reg.peak)
    b.update(still)
    moved.update(volumes)
    sa, sb, sm = (crop(m.finish("std")[0]) for m in (a, b, moved))
    assert same_bits(sa, sb), "the activity map of the registered series is the still scene's on the box"
    assert not same_bits(sm, sb), "the unregistered series' is not"
    one = registrar(volumes[5])
    assert tuple(one.shape) == shape and same_bits(one, reg.volumes[5]) and len(registrar.peak) == 3, "one volume"


# With the stack's own median as template the limit of section 26.4 holds here too, and sooner: 6 volumes are fewer than the 8 frames
# there.  On this scene with 4 of 6 volumes at rest, the restatement estimates 0 for the two moved volumes at smooth = 0 (their own
# noise survives in the median and correlates with itself at shift 0; second peak / peak 0.46 - 0.94 with a low-pass of 0.3 - 1
# voxels, no width recovered both).  The resting volumes are found at rest with a wide margin (second peak / peak <= 0.16), which is
# asserted; of the moved ones only what holds whatever the estimate: n_iter = 2 takes the median of the FIRST pass's stack, moves the
# ORIGINAL volumes once, and repeats bit for bit.
@pytest.mark.parametrize("seed", [0, 1])
def test_two_iterations_from_the_stack_own_median(seed):
    from cwfa_amd.CWFA import register_volumes
    sc = planted(seed, rest=3)
    assert not sc.shifts[:4].any() and sc.shifts[4:].any(axis=1).all(), "4 of 6 volumes rest"
    volumes = dev(sc.volumes)
    kw = dict(subpixel=False, mode="nearest", **KW)
    reg = register_volumes(volumes, None, n_iter=2, **kw)
    s = reg.shifts.cpu().numpy()
    assert not s[:4].any(), "the resting volumes are found at rest"
    assert tuple(reg.template.shape) == sc.volumes.shape[1:] and reg.template.dtype == torch.float32
    one = register_volumes(volumes, None, n_iter=1, **kw)
    assert same_bits(one.template, R.lower_median(sc.volumes)), "the first template is the stack's lower median"
    assert same_bits(reg.template, R.lower_median(one.volumes.cpu().numpy())), "the second is the median of the FIRST pass's stack"
    assert same_bits(reg.volumes, R3.shift(sc.volumes, s, "nearest")), "and the volumes are the originals moved once"
    again = register_volumes(volumes, None, n_iter=2, **kw)
    assert same_bits(again.volumes, reg.volumes) and same_bits(again.shifts, reg.shifts) and same_bits(again.peak, reg.peak)


# The largest |device - restatement| of the sub-voxel shifts over CASES x seeds 0 .. 2, observed on the MI355X: 2.384e-07 voxels at
# either size -- one unit in the last place of an fp32 shift between 2 and 4.  The two differ only in the transforms (rocFFT in fp32
# against numpy.fft in float64), whose rounding reaches the shift through the parabola's denominator.  The bound is 4 x the
# observation, the margin section 26.4 uses for that.
OBSERVED_SUBVOXEL_DIFF = 2.384e-07
SUBVOXEL_DIFF_BOUND = 4.0 * OBSERVED_SUBVOXEL_DIFF


@pytest.mark.parametrize("shape,max_d,taper", CASES)
def test_subvoxel_shifts_against_the_restatement(shape, max_d, taper):
    from cwfa_amd.CWFA import estimate_volume_shifts
    worst = 0.0
    m = tuple(v + 1 for v in max_d)
    for seed in (0, 1, 2):
        sc = planted(seed, shape, max_d, True)
        c = R3.correlate(sc.volumes, sc.template, taper)
        want, wi, wpk = R3.peak(c, m, True)
        got, pk = estimate_volume_shifts(dev(sc.volumes), dev(sc.template), max_shift=m, taper=taper, chunk=2)
        got = got.cpu().numpy()
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.all(np.abs(got - wi) <= 0.5), "the same integer peak: the refinement moves it by at most half a voxel"
        assert float(np.abs(pk.cpu().numpy() - wpk).max()) < 1e-3
    print(f"{shape}: largest |device - restatement| of the sub-voxel shifts = {worst:.3e} voxels")
    assert worst <= SUBVOXEL_DIFF_BOUND
