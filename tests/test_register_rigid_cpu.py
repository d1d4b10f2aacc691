"""Rigid registration of volumes with a rotation about the optical axis without a GPU: the rigid fit of a table
of block shifts, its rejection pass, its degenerate tables and its composition with a prior motion on the numpy restatement
(tests/register_rigid_ref.py), the restatement of the resampling against the rigid shift, exact copies and quarter turns, the corner
rule of the valid box, the planted scene end to end, the argument validation of the two entry points through the built library, and
the refusals the Python layer decides before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import register3d_ref as R3
import register_rigid_ref as RR

F32, F64 = np.float32, np.float64
u32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
# the planted scene of the issue: 6 volumes of 8 x 64 x 72, blocks of 8 x 32 x 36 on a 1 x 3 x 3 grid, |theta| <= 3 degrees, |d| <= 2
E2E = dict(shape=(8, 64, 72), block=(8, 32, 36), grid=(1, 3, 3), N=6, max_deg=3.0, max_d=2.0)
E2E_EST = dict(n_refine=2, max_shift=(1, 6, 6), taper=(1, 4, 4))
E2E_SEEDS = tuple(range(8))


@pytest.fixture(scope="module")
def L():
    from cwfa_amd import _lib, build
    build.build_all()
    return _lib.lib()


@pytest.fixture(scope="module")
def ptr():
    buf = ctypes.create_string_buffer(32768)
    base = ctypes.addressof(buf)
    return ctypes.c_void_p((base + 15) & ~15)


def motions(rng, n, max_theta=0.3, max_d=3.0):
    th = rng.uniform(-max_theta, max_theta, n)
    return np.stack((rng.uniform(-1, 1, n), rng.uniform(-max_d, max_d, n), rng.uniform(-max_d, max_d, n), np.cos(th), np.sin(th)), axis=1)


def matrix_compose(A, B):
    """A o B written with matrices: rotation R_A R_B, shift R_A d_B + d_A, dz added."""
    RA, RB = (np.array([[p[3], -p[4]], [p[4], p[3]]]) for p in (A, B))
    Rt, d = RA @ RB, RA @ B[1:3] + A[1:3]
    return np.array([A[0] + B[0], d[0], d[1], Rt[0, 0], Rt[1, 0]])


# ------------------------------------------------------------------------------------------------ the fit
def test_exact_tables_come_back():
    G = RR.block_grid((8, 64, 72), (8, 32, 36), (1, 3, 3))
    a = RR.arms(G)
    P = motions(np.random.default_rng(0), 200)
    got, inl = RR.fit(RR.table_of(P, a, F64), np.ones((200, 9), dtype=F32), a, dtype=F64)
    worst = np.abs(got - P).max()
    print(f"exact tables: largest parameter error {worst:.2e}")
    assert inl.all() and worst <= 1e-12
    assert np.abs(got[:, 3] ** 2 + got[:, 4] ** 2 - 1).max() <= 4e-16
    # the measured table is fp32: the same motions through a table rounded once stay within that rounding times the lever arm
    got32, _ = RR.fit(RR.table_of(P, a), np.ones((200, 9), dtype=F32), a)
    assert np.abs(got32 - P).max() <= 1e-6
    # a grid with gz > 1: all blocks vote for one rotation and one dz
    G2 = RR.block_grid((16, 64, 72), (8, 32, 36), (2, 3, 3))
    a2 = RR.arms(G2)
    assert a2.shape == (18, 2) and np.array_equal(a2[:9], a2[9:]) and np.array_equal(a2[:9], a)
    got2, _ = RR.fit(RR.table_of(P[:20], a2, F64), np.ones((20, 18), dtype=F32), a2, dtype=F64)
    assert np.abs(got2 - P[:20]).max() <= 1e-12


def test_two_moved_blocks_are_rejected_and_the_fit_is_the_fit_without_them():
    G = RR.block_grid((8, 64, 72), (8, 32, 36), (1, 3, 3))
    a = RR.arms(G)
    P = motions(np.random.default_rng(1), 12, 0.05)
    t = RR.table_of(P, a)
    moved = t.copy()
    moved[:, 2, 1] += 3.0
    moved[:, 6, 2] -= 3.0
    pk = np.ones((12, 9), dtype=F32)
    got, inl = RR.fit(moved, pk, a)
    without = pk.copy()
    without[:, [2, 6]] = np.nan
    want, inl2 = RR.fit(moved, without, a)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.array_equal(inl, inl2)
    assert not inl[:, [2, 6]].any() and inl.sum() == 12 * 7 and np.abs(got - P).max() <= 1e-6
    # reject = inf switches the pass off: the moved blocks pull the fit
    loose, inl3 = RR.fit(moved, pk, a, reject=np.inf)
    assert inl3.all() and np.abs(loose - P).max() > 0.1
    # every block beyond `reject` of a first fit none of them agrees with: the first fit and the first weights stand
    wild = np.zeros((1, 2, 3), dtype=F32)
    wild[0, 0, 0], wild[0, 1, 0] = 5.0, -5.0
    p, i = RR.fit(wild, np.ones((1, 2), dtype=F32), np.array([[0.0, -1.0], [0.0, 1.0]]))
    assert i.all() and p[0, 0] == 0.0


def test_degenerate_tables():
    G = RR.block_grid((8, 64, 72), (8, 32, 36), (1, 3, 3))
    a = RR.arms(G)
    P = motions(np.random.default_rng(2), 4, 0.1)
    t, pk = RR.table_of(P, a), np.ones((4, 9), dtype=F32)
    # m = 0
    got, inl = RR.fit(t, np.full((4, 9), np.nan, dtype=F32), a)
    assert np.array_equal(got, np.tile(RR.IDENTITY, (4, 1))) and not inl.any()
    got, inl = RR.fit(t, pk * F32(0.2), a, min_peak=0.5)
    assert np.array_equal(got, np.tile(RR.IDENTITY, (4, 1))) and not inl.any()
    # one block of nine: no angle, its own shift
    one = np.full((4, 9), -np.inf, dtype=F32)
    one[:, 4] = 1.0
    got, inl = RR.fit(t, one, a)
    assert np.array_equal(got[:, 3:], np.tile([1.0, 0.0], (4, 1))) and np.array_equal(got[:, :3], t[:, 4].astype(F64)) and inl.sum() == 4
    # B = 1
    got, inl = RR.fit(t[:, :1], pk[:, :1], a[:1])
    assert np.array_equal(got[:, 3:], np.tile([1.0, 0.0], (4, 1))) and np.array_equal(got[:, :3], t[:, 0].astype(F64)) and inl.all()
    # coincident centres: no angle, the mean shift
    got, _ = RR.fit(t[:, :2], pk[:, :2], np.tile(a[:1], (2, 1)), reject=np.inf)
    assert np.array_equal(got[:, 3:], np.tile([1.0, 0.0], (4, 1)))
    # collinear centres still give the angle
    G3 = RR.block_grid((8, 64, 72), (8, 32, 36), (1, 1, 3))
    a3 = RR.arms(G3)
    assert (a3[:, 0] == a3[0, 0]).all()
    got, inl = RR.fit(RR.table_of(P, a3, F64), pk[:, :3], a3, dtype=F64)
    assert inl.all() and np.abs(got - P).max() <= 1e-12
    # a NaN shift or peak is skipped: the fit of the rest
    holes, hp = t.copy(), pk.copy()
    holes[:, 1, 2], holes[:, 5, 0], hp[:, 7] = np.nan, np.inf, np.nan
    got, inl = RR.fit(holes, hp, a)
    assert not inl[:, [1, 5, 7]].any() and inl.sum() == 4 * 6 and np.abs(got - P).max() <= 1e-6
    # P <= 0 (a table that asks for more than a quarter turn): the identity rotation and the mean shift
    far = np.array([[0.0, 0.5, -0.25, np.cos(2.0), np.sin(2.0)]])
    got, _ = RR.fit(RR.table_of(far, a), pk[:1], a, reject=np.inf)
    assert got[0, 3] == 1.0 and got[0, 4] == 0.0 and np.isfinite(got).all()


def test_composition_with_a_prior():
    G = RR.block_grid((8, 64, 72), (8, 32, 36), (1, 3, 3))
    a = RR.arms(G)
    rng = np.random.default_rng(3)
    A, B = motions(rng, 50), motions(rng, 50, 0.1)
    got, _ = RR.fit(RR.table_of(B, a, F64), np.ones((50, 9), dtype=F32), a, prior=A, dtype=F64)
    want = np.array([matrix_compose(p, q) for p, q in zip(A, B)])
    worst = np.abs(got - want).max()
    print(f"composition: largest difference to the matrix product {worst:.2e}")
    assert worst <= 1e-12
    # the identity as prior changes nothing but the last bit of the normalisation
    plain, _ = RR.fit(RR.table_of(B, a, F64), np.ones((50, 9), dtype=F32), a, dtype=F64)
    ident, _ = RR.fit(RR.table_of(B, a, F64), np.ones((50, 9), dtype=F32), a, prior=np.tile(RR.IDENTITY, (50, 1)), dtype=F64)
    assert np.abs(plain - ident).max() <= 4e-16
    # what the composition means: moving under A, then under B, is moving under A o B.  On a ramp (interpolation is exact on an
    # affine function, up to fp32 rounding of values below 256: a few 1e-5 per operation) the two agree away from the border,
    # and the other order does not
    Y, X = np.meshgrid(np.arange(24.0), np.arange(24.0), indexing="ij")
    x = np.broadcast_to(3.0 * Y + 5.0 * X + 7.0, (1, 2, 24, 24)).astype(F32)
    pa, pb = np.array([[0, 1.0, -2.0, np.cos(0.05), np.sin(0.05)]]), np.array([[0, -1.5, 1.0, np.cos(-0.03), np.sin(-0.03)]])
    twice = RR.move(RR.move(x, pa), pb)
    once = RR.move(x, np.array([RR.compose(pa[0], tuple(pb[0]))]))
    other = RR.move(x, np.array([RR.compose(pb[0], tuple(pa[0]))]))
    assert np.abs(twice - once)[:, :, 6:18, 6:18].max() < 1e-3 and np.abs(twice - other)[:, :, 6:18, 6:18].min() > 0.1


# ------------------------------------------------------------------------------------------------ the resampling
def test_no_rotation_is_the_rigid_shift_bit_for_bit():
    rng = np.random.default_rng(5)
    x = rng.uniform(-50, 200, (5, 3, 6, 9)).astype(F32)
    d = np.array([[0.5, 1.25, -2.75], [0.0, 0.3, 0.6], [-1.0, 2.0, -3.0], [1.5, -0.125, 0.0], [-1e-10, 7.5, 0.5]], dtype=F64)
    p = np.concatenate((d, np.tile([1.0, 0.0], (5, 1))), axis=1)
    for mode in ("bilinear", "nearest"):
        for c0 in (None, (1.5, 7.0)):
            assert np.array_equal(u32(RR.move(x, p, c0, mode, fill=-3.5)), u32(R3.shift(x, d.astype(F32), mode, fill=-3.5))), (mode, c0)


def test_integer_shifts_copy_bits_and_quarter_turns_are_rot90():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, 3, 8, 8)).astype(F32)
    x[0, 1, 2, 3], x[1, 0, 5, 5], x[1, 2, 0, 7] = np.nan, np.inf, -0.0
    p = np.array([[1.0, -2.0, 3.0, 1.0, 0.0], [-1.0, 0.0, 1.0, 1.0, 0.0]])
    got = RR.move(x, p, fill=9.0)
    for n, (dz, dy, dx) in enumerate(((1, -2, 3), (-1, 0, 1))):
        for z in range(3):
            for y in range(8):
                for xx in range(8):
                    zz, yy, xs = z + dz, y + dy, xx + dx
                    want = x[n, zz, yy, xs] if 0 <= zz < 3 and 0 <= yy < 8 and 0 <= xs < 8 else F32(9.0)
                    assert u32(got[n, z, y, xx]) == u32(want)
    # (c, s) = (0, +-1) about the centre of a square plane: every tap lands on an integer position
    q = np.array([[0.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0, -1.0]])
    turned = RR.move(x, q)
    assert np.array_equal(u32(turned[0]), u32(np.rot90(x[0], k=-1, axes=(1, 2)))) and np.array_equal(u32(turned[1]), u32(np.rot90(x[1], k=1, axes=(1, 2))))
    # odd side: the centre is a voxel
    y7 = rng.standard_normal((1, 2, 7, 7)).astype(F32)
    assert np.array_equal(u32(RR.move(y7, q[:1])[0]), u32(np.rot90(y7[0], k=-1, axes=(1, 2))))


def test_nearest_and_parameters_that_are_not_finite():
    rng = np.random.default_rng(7)
    x = rng.uniform(0, 10, (1, 4, 10, 12)).astype(F32)
    th = np.radians(7.0)
    p = np.array([[0.6, 1.4, -0.7, np.cos(th), np.sin(th)]])
    near = RR.move(x, p, mode="nearest", fill=-1.0)
    dzf, v = RR.displacement(p[0], (4, 10, 12))
    for z in range(4):
        for y in range(10):
            for xx in range(12):
                zz, yy, xs = z + int(np.rint(dzf)), y + int(np.rint(v[y, xx, 0])), xx + int(np.rint(v[y, xx, 1]))
                want = x[0, zz, yy, xs] if 0 <= zz < 4 and 0 <= yy < 10 and 0 <= xs < 12 else F32(-1.0)
                assert u32(near[0, z, y, xx]) == u32(want)
    for k in range(5):
        for bad in (np.nan, np.inf, -np.inf):
            q = p.copy()
            q[0, k] = bad
            assert (RR.move(x, q, fill=2.5) == F32(2.5)).all(), (k, bad)
    q = p.copy()
    q[0, 1] = 1e30                                                         # finite in fp32: every tap is outside and reads the fill
    assert (RR.move(x, q, mode="nearest", fill=2.5) == F32(2.5)).all()
    q[0, 1] = 1e300                                                        # not finite once rounded to fp32
    assert (RR.move(x, q, fill=2.5) == F32(2.5)).all()


def test_corner_shifts_feed_the_valid_box():
    from cwfa_amd.CWFA import rigid_corner_shifts, valid_box
    rng = np.random.default_rng(8)
    shape = (4, 20, 26)
    P = motions(rng, 6, 0.12, 2.5)
    P[:, 0] = rng.uniform(-1.2, 1.2, 6)
    for c0 in (None, (3.3, 17.0)):
        cs = RR.corner_shifts(P, shape, c0)
        got = rigid_corner_shifts(torch.from_numpy(P), shape, c0)
        assert got.dtype == torch.float32 and tuple(got.shape) == (24, 3) and np.array_equal(u32(got.numpy()), u32(cs))
        # the displacement is monotone along each axis, rounding included: its extremes over the plane are at the corners
        for n in range(6):
            dzf, v = RR.displacement(P[n], shape, c0)
            for k in (0, 1):
                assert v[..., k].min() == cs[4 * n:4 * n + 4, 1 + k].min() and v[..., k].max() == cs[4 * n:4 * n + 4, 1 + k].max()
        box = valid_box(got, shape)
        assert box == R3.valid_box(cs, shape) and box[1] > box[0] and box[3] - box[2] >= 8 and box[5] - box[4] >= 12
        moved = RR.move(np.ones((6, *shape), dtype=F32), P, c0, fill=np.nan)
        z0, z1, y0, y1, x0, x1 = box
        assert np.isfinite(moved[:, z0:z1, y0:y1, x0:x1]).all() and not np.isfinite(moved).all()
    bad = P.copy()
    bad[2, 3] = np.nan
    assert valid_box(rigid_corner_shifts(torch.from_numpy(bad), shape), shape) == (0,) * 6
    assert valid_box(rigid_corner_shifts(torch.zeros(0, 5, dtype=torch.float64), shape), shape) == (0, 4, 0, 20, 0, 26)
    with pytest.raises(ValueError, match="params"):
        rigid_corner_shifts(torch.zeros(3, 4), shape)
    with pytest.raises(ValueError, match="shape"):
        rigid_corner_shifts(torch.zeros(3, 5), (20, 26))
    with pytest.raises(ValueError, match="center"):
        rigid_corner_shifts(torch.zeros(3, 5), shape, (1.0, float("inf")))


# ------------------------------------------------------------------------------------------------ the planted scene, end to end
def test_the_planted_scene_end_to_end():
    """(a) the angle of every volume comes back within the lever-arm bound of half a voxel of error per block shift, 1.35 degrees for
    this grid; (b) per seed the registered stack is closer to the still scene than section 30's translation-only registration of the
    same volumes.  MEASURED over seeds 0 .. 7: the worst angle error after passes 1, 2, 3 is 0.592, 0.374, 0.257 degrees; the
    mean absolute difference to the still scene is 0.51 .. 0.75 of the translation-only one."""
    bound = np.degrees(RR.lever_bound(RR.block_grid(E2E["shape"], E2E["block"], E2E["grid"])))
    assert abs(bound - 1.3528) < 1e-3
    worst, ratios = np.zeros(E2E_EST["n_refine"] + 1), []
    for seed in E2E_SEEDS:
        sc = RR.scene(seed, **E2E)
        assert not sc.params[0, :3].any() and np.abs(RR.angles(sc.params)).max() <= 3.0
        params, peak, inlier, shifts, history = RR.estimate(sc.volumes, sc.template, sc.grid, **E2E_EST)
        true = RR.angles(sc.params)
        errs = np.array([np.abs(RR.angles(h) - true).max() for h in history])
        worst = np.maximum(worst, errs)
        moved = RR.move(sc.volumes, params)
        plain, s = RR.translation_only(sc.volumes, sc.template, E2E_EST["max_shift"], E2E_EST["taper"])
        box = RR.both_boxes(params, s, E2E["shape"])
        rigid, trans = RR.valid_mean_abs(moved, sc.still, box), RR.valid_mean_abs(plain, sc.still, box)
        ratios.append(rigid / trans)
        print(f"seed {seed}: angle error per pass {np.round(errs, 3)} deg, rigid {rigid:.2f} / translation only {trans:.2f} counts on {box}")
        assert np.abs(RR.angles(params) - true).max() < bound, f"seed {seed}"
        assert box[1] - box[0] >= 4 and box[3] - box[2] >= 48 and box[5] - box[4] >= 56 and rigid < trans, f"seed {seed}"
    print(f"worst angle error per pass {np.round(worst, 3)} deg (bound {bound:.3f}); rigid / translation only {min(ratios):.2f} .. {max(ratios):.2f}")


def test_the_planted_motion_gives_back_the_still_scene():
    sc = RR.scene(0, **E2E)
    moved = RR.move(sc.volumes, sc.params)
    # the sign convention: the planted parameters undo the motion, the opposite angle and shift double it (what is left after the
    # planted motion is the noise of the canvas, interpolated twice: no threshold is put on it)
    wrong = sc.params * np.array([1.0, -1.0, -1.0, 1.0, -1.0])
    box = R3.valid_box(np.concatenate((RR.corner_shifts(sc.params, E2E["shape"]), RR.corner_shifts(wrong, E2E["shape"]))), E2E["shape"])
    plain = RR.valid_mean_abs(sc.volumes, sc.still, box)
    back = RR.valid_mean_abs(moved, sc.still, box)
    worse = RR.valid_mean_abs(RR.move(sc.volumes, wrong), sc.still, box)
    print(f"planted motion undone: {back:.2f} counts against {plain:.2f} unregistered and {worse:.2f} under the opposite motion")
    assert back < plain < worse


# ------------------------------------------------------------------------------------------------ the entry points' arguments
def test_reg_fit_rigid_arguments(L, ptr):
    s, pk, a, prior, params, inl = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(6))

    def call(s=s, pk=pk, a=a, N=2, B=4, min_peak=0.1, reject=1.0, prior=prior, params=params, inl=inl):
        return L.cwfa_reg_fit_rigid_f64(s, pk, a, N, B, min_peak, reject, prior, params, inl, None)

    for k in ("s", "pk", "a", "params", "inl"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_fit_rigid_f64: null" in L.cwfa_last_error(), k
    assert call(N=-1) == -2 and b"negative" in L.cwfa_last_error()
    for B in (0, -1, 4097):
        assert call(B=B) == -2 and b"blocks" in L.cwfa_last_error(), B
    for kw in ({"min_peak": -0.5}, {"min_peak": float("nan")}, {"reject": -1.0}, {"reject": float("nan")}):
        assert call(**kw) == -1 and b"min_peak and reject" in L.cwfa_last_error(), kw
    for k in ("a", "prior", "params"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 16384 + 4)}) == -3 and b"8-byte" in L.cwfa_last_error(), k
    for k in ("s", "pk"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 16384 + 2)}) == -3 and b"4-byte" in L.cwfa_last_error(), k
    assert call(prior=params) == -1 and b"alias" in L.cwfa_last_error()
    assert call(N=0) == 0 and call(N=0, prior=None) == 0 and call(N=0, reject=float("inf"), B=4096) == 0, "empty: no launch"


def test_reg_rigid3d_arguments(L, ptr):
    x, p, out = (ctypes.c_void_p(ptr.value + 4096 * k) for k in range(3))

    def call(x=x, N=2, D=3, H=4, W=8, vs=96, p=p, cy=1.5, cx=3.5, mode=0, fill=0.0, out=out):
        return L.cwfa_reg_rigid3d_f32(x, N, D, H, W, vs, p, cy, cx, mode, fill, out, None)

    for k in ("x", "p", "out"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_rigid3d_f32: null" in L.cwfa_last_error(), k
    assert call(mode=2) == -1 and call(mode=-1) == -1 and b"mode" in L.cwfa_last_error()
    for kw in ({"cy": float("nan")}, {"cx": float("inf")}, {"cy": -float("inf")}):
        assert call(**kw) == -1 and b"centre" in L.cwfa_last_error(), kw
    assert call(N=-1) == -2 and call(D=-1) == -2 and call(H=-1) == -2 and call(W=-1) == -2 and b"negative" in L.cwfa_last_error()
    assert call(D=1 << 10, H=1 << 11, W=1 << 10) == -2 and call(W=1 << 30, D=1, H=1) == -2 and b"too large" in L.cwfa_last_error()
    for k in ("x", "out"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 16384 + 2)}) == -3 and b"4-byte" in L.cwfa_last_error(), k
    assert call(p=ctypes.c_void_p(ptr.value + 16384 + 4)) == -3 and b"8-byte" in L.cwfa_last_error()
    assert call(vs=95) == -1 and call(vs=-97) == -1 and b"stride" in L.cwfa_last_error()
    assert call(out=x) == -1 and b"alias" in L.cwfa_last_error()
    assert call(N=0) == 0 and call(D=0, vs=0) == 0 and call(H=0, vs=0) == 0 and call(W=0, vs=0) == 0, "empty: no launch"


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_python_layer_refuses_before_any_device_work():
    from cwfa_amd import ops
    from cwfa_amd.CWFA import (RigidVolumeRegistrar, block_grid, estimate_rigid_motion, fit_rigid_motion, register_volumes_rigid, rigid_angles,
                               rigid_move_volumes)
    v, t = torch.zeros(4, 6, 40, 48), torch.zeros(6, 40, 48)
    G = block_grid((6, 40, 48), (6, 20, 24))
    p = torch.zeros(4, 5, dtype=torch.float64)
    s, pk = torch.zeros(4, 1, 2, 2, 3), torch.zeros(4, 1, 2, 2)
    for call in (lambda: estimate_rigid_motion(v[..., ::2], t[..., ::2], G), lambda: register_volumes_rigid(v[:, :, ::2]), lambda: rigid_move_volumes(v[..., ::2], p),
                 lambda: estimate_rigid_motion(v[0], t, G), lambda: register_volumes_rigid(v[0]), lambda: rigid_move_volumes(v[0], p)):
        with pytest.raises(ValueError, match=r"contiguous \[N,D,H,W\]"):
            call()
    for call in (lambda: estimate_rigid_motion(v.half(), t, G), lambda: register_volumes_rigid(v.double(), t), lambda: rigid_move_volumes(v.half(), p)):
        with pytest.raises(ValueError, match="float32 stack"):
            call()
    for bad in (torch.zeros(6, 40, 47), torch.zeros(6, 40, 48, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="template"):
            estimate_rigid_motion(v, bad, G)
    for fn in (lambda **k: estimate_rigid_motion(v, t, G, **k), lambda **k: register_volumes_rigid(v, t, **k)):
        with pytest.raises(ValueError, match="'dft'.*not built"):
            fn(subpixel="dft")
        for kw in ({"min_peak": float("nan")}, {"min_peak": -1.0}, {"reject": float("nan")}, {"reject": -0.5}):
            with pytest.raises(ValueError, match="min_peak and reject"):
                fn(**kw)
        with pytest.raises(ValueError, match="chunk"):
            fn(chunk=0)
        with pytest.raises(ValueError, match="n_refine"):
            fn(n_refine=-1)
        for c in ((1.0,), "x", (1.0, float("nan")), (0.0, 1.0, 2.0)):
            with pytest.raises(ValueError, match="center"):
                fn(center=c)
    for bad in ((1, 2, 2), None, block_grid((6, 40, 50), (6, 20, 24))):
        with pytest.raises(ValueError, match="grid"):
            estimate_rigid_motion(v, t, bad)
    with pytest.raises(ValueError, match="grid"):
        fit_rigid_motion(s, pk, (1, 2, 2))
    for m in ((3, 8, 8), (2, 10, 8), (2, 8, 12), (2, 8)):                  # against the BLOCK: 6 x 20 x 24
        with pytest.raises(ValueError, match="max_shift.*block"):
            estimate_rigid_motion(v, t, G, max_shift=m)
    for tp in ((4, 0, 0), (0, 11, 0), (0, 0, 13)):
        with pytest.raises(ValueError, match="taper.*block"):
            estimate_rigid_motion(v, t, G, taper=tp)
    for bad in (torch.zeros(4, 5), torch.zeros(3, 5, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="params"):
            rigid_move_volumes(v, bad)
    with pytest.raises(ValueError, match="mode"):
        rigid_move_volumes(v, p, mode="cubic")
    with pytest.raises(ValueError, match="center"):
        rigid_move_volumes(v, p, center=(1.0, float("inf")))
    for out in (v, v[:], v[1:]):
        with pytest.raises(ValueError, match="alias"):
            rigid_move_volumes(v, p, out=out)
    with pytest.raises(ValueError, match="alias"):
        register_volumes_rigid(v, t, out=v)
    with pytest.raises(ValueError, match="n_iter"):
        register_volumes_rigid(v, t, n_iter=0)
    for bad in (torch.zeros(4, 1, 2, 2, 2), torch.zeros(4, 5, 3), torch.zeros(4, 4, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="shifts"):
            fit_rigid_motion(bad, pk, G)
    for bad in (torch.zeros(4, 3), torch.zeros(4, 4, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="peak"):
            fit_rigid_motion(s, bad, G)
    for bad in (torch.zeros(4, 5), torch.zeros(3, 5, dtype=torch.float64)):
        with pytest.raises(ValueError, match="prior"):
            fit_rigid_motion(s, pk, G, prior=bad)
    for kw in ({"min_peak": float("nan")}, {"reject": -1.0}):
        with pytest.raises(ValueError, match="min_peak and reject"):
            fit_rigid_motion(s, pk, G, **kw)
        with pytest.raises(ValueError, match="min_peak and reject"):
            ops.reg_fit_rigid(s.reshape(4, 4, 3), pk.reshape(4, 4), torch.zeros(4, 2, dtype=torch.float64), **kw)
    with pytest.raises(ValueError, match="shifts"):
        ops.reg_fit_rigid(torch.zeros(4, 4, 2), pk.reshape(4, 4), torch.zeros(4, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="blocks"):
        ops.reg_fit_rigid(torch.zeros(1, 4097, 3), torch.zeros(1, 4097), torch.zeros(4097, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="mode"):
        ops.reg_rigid3d(v, p, mode="cubic")
    with pytest.raises(ValueError, match="center"):
        ops.reg_rigid3d(v, p, center=(1.0,))
    with pytest.raises(ValueError, match="stack"):
        ops.reg_rigid3d(v[0], p)
    with pytest.raises(ValueError, match="params"):
        rigid_angles(torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RigidVolumeRegistrar(t, G)
    for call in (lambda: estimate_rigid_motion(v, t, G), lambda: rigid_move_volumes(v, p), lambda: register_volumes_rigid(v, t), lambda: fit_rigid_motion(s, pk, G),
                 lambda: ops.reg_fit_rigid(s.reshape(4, 4, 3), pk.reshape(4, 4), torch.zeros(4, 2, dtype=torch.float64)), lambda: ops.reg_rigid3d(v, p)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert torch.allclose(rigid_angles(torch.tensor([[0, 0, 0, 0.0, 1.0], [0, 0, 0, 1.0, 0.0]], dtype=torch.float64)), torch.tensor([90.0, 0.0], dtype=torch.float64))


def test_the_names_are_exported_and_existing_estimators_keep_their_helper():
    from cwfa_amd import CWFA
    for name in ("fit_rigid_motion", "RigidFit", "rigid_move_volumes", "estimate_rigid_motion", "register_volumes_rigid", "RigidRegistration",
                 "RigidVolumeRegistrar", "rigid_angles", "rigid_corner_shifts"):
        assert name in CWFA.__all__ and hasattr(CWFA, name)
    assert CWFA.RigidRegistration._fields == ("volumes", "params", "peak", "inlier", "shifts", "template")
    assert CWFA.RigidFit._fields == ("params", "inlier")
    assert "valid_box(rigid_corner_shifts(params, shape, center), shape)" in CWFA.rigid_move_volumes.__doc__
    # the arms the Python layer builds are the restatement's
    G = CWFA.block_grid((16, 64, 72), (8, 32, 36), (2, 3, 3))
    for c0 in (None, (3.3, 40.0)):
        got = CWFA._rigid_arms(G, CWFA._rigid_center(c0, G.shape, "test"), "cpu").numpy()
        assert np.array_equal(got, RR.arms(RR.block_grid((16, 64, 72), (8, 32, 36), (2, 3, 3)), c0))
