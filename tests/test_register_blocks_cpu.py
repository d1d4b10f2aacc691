"""Piecewise-rigid registration of volumes without a GPU: the grid of blocks and its interpolation tables, the
lerp, the clean-up rule and the warp of the numpy restatement (tests/register_blocks_ref.py), the planted piecewise-constant scene
with its second-peak cap, the argument validation of the three entry points through the built library, and the refusals the Python
layer decides before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import register3d_ref as R3
import register_blocks_ref as RB

F32 = np.float32
u32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
# (shape, grid) of scene (P); the blocks are section 30.4's tested size, 12 x 24 x 28, |d| <= (2, 3, 3), the window one wider
P_CASES = (((12, 48, 56), (1, 2, 2)), ((24, 48, 56), (2, 2, 2)))
P_BLOCK, P_MAX_D, P_TAPER = (12, 24, 28), (2, 3, 3), (1, 3, 3)
# the seeds of scene (P), for which the restatement alone meets the cap below on every block (checked here); MEASURED over them, per
# shape: the largest correlation value outside the 3 x 3 x 3 around a block's peak over the peak, 0.364 and 0.373 (the cap is what
# lets the device test demand the exact table although rocFFT and numpy round differently)
P_SEEDS = (0, 1, 2, 3)
CAP = 0.5


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


# ------------------------------------------------------------------------------------------------ the grid
def test_origins_centres_and_tables_written_out():
    # overlapping: 10 voxels, blocks of 4, 4 blocks -> origins 0, 2, 4, 6
    o, c, idx, t = RB.axis_grid(10, 4, 4)
    assert o.tolist() == [0, 2, 4, 6] and c.tolist() == [1.5, 3.5, 5.5, 7.5]
    assert idx.tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 3, 3]
    assert np.array_equal(t, np.array([0, 0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0, 0], dtype=F32))
    # gapped: 11 voxels, blocks of 2, 3 blocks -> origins 0, 4, 9 (integer division), a gap between them
    o, c, idx, t = RB.axis_grid(11, 2, 3)
    assert o.tolist() == [0, 4, 9] and c.tolist() == [0.5, 4.5, 9.5]
    assert idx.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2] and t[0] == 0 and t[10] == 0 and t[1] == F32(0.5 / 4.0) and t[5] == F32(0.5 / 5.0)
    # one block: centred, every coordinate takes node 0
    o, c, idx, t = RB.axis_grid(9, 4, 1)
    assert o.tolist() == [2] and c.tolist() == [3.5] and not idx.any() and not t.any()
    # a block as large as the axis: every origin 0, every centre equal, no coordinate strictly between two centres
    o, c, idx, t = RB.axis_grid(6, 6, 3)
    assert o.tolist() == [0, 0, 0] and c.tolist() == [2.5] * 3 and idx.tolist() == [0, 0, 0, 2, 2, 2] and not t.any()
    # a coordinate exactly on an end centre (odd block): node 0 / the last node with t = 0, and an inner centre gives t = 0 there
    o, c, idx, t = RB.axis_grid(9, 3, 3)
    assert c.tolist() == [1.0, 4.0, 7.0] and idx.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2] and t[1] == 0 and t[4] == 0 and t[7] == 0


@pytest.mark.parametrize("shape,block,grid", [((12, 48, 56), (12, 24, 28), (1, 2, 2)), ((10, 11, 9), (4, 2, 3), (4, 3, 3)), ((7, 9, 13), (7, 4, 5), (3, 1, 4)),
                                              ((5, 6, 7), (32, 128, 128), None), ((96, 512, 512), (32, 128, 128), None), ((9, 40, 33), (3, 7, 5), (1, 9, 1))])
def test_block_grid_is_the_restatement(shape, block, grid):
    from cwfa_amd.CWFA import block_grid
    G, H = RB.block_grid(shape, block, grid), block_grid(shape, block, grid)
    assert H.shape == G.shape and H.block == G.block and H.grid == G.grid and H.B == int(np.prod(G.grid))
    for a in range(3):
        assert np.array_equal(H.origins[a], G.origins[a]) and H.origins[a].dtype == np.int32
        assert np.array_equal(H.centers[a], G.centers[a]) and H.centers[a].dtype == np.float64
        assert np.array_equal(H.idx[a], G.idx[a]) and H.idx[a].dtype == np.int32
        assert np.array_equal(u32(H.t[a]), u32(G.t[a])) and H.t[a].dtype == np.float32
        assert (G.origins[a] >= 0).all() and (G.origins[a] <= shape[a] - G.block[a]).all()
        assert (G.t[a] >= 0).all() and (G.t[a] < 1).all() and (G.t[a][G.idx[a] == G.grid[a] - 1] == 0).all(), "node i + 1 is never needed past the grid"
    if grid is None:
        assert G.grid == tuple(-(-s // b) for s, b in zip(shape, G.block)) and all(b <= s for b, s in zip(G.block, shape))


# ------------------------------------------------------------------------------------------------ the lerp
def test_lerp_is_exact_for_equal_nodes_and_for_t_zero():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-30, 30, 2000), [0.0, 1e30, -1e30, 3.0, -7.0]]).astype(F32)
    t = np.concatenate([rng.random(2000), [0.5, 0.25, 0.999, 1e-7, 0.3]]).astype(F32)
    assert np.array_equal(RB.lerp(a, a, t), a), "a + t (a - a) is a: a constant field is the rigid shift"
    b = np.roll(a, 1)
    assert np.array_equal(u32(RB.lerp(a, b, np.zeros_like(t))), u32(a))
    assert np.array_equal(u32(RB.lerp(a, np.full_like(a, np.nan), np.zeros_like(t))), u32(a)), "t == 0 does not look at b"
    assert RB.lerp(F32(1), F32(3), F32(0.5)) == F32(2) and RB.lerp(F32(2), F32(-2), F32(0.25)) == F32(1)


# ------------------------------------------------------------------------------------------------ the clean-up
def _table(grid, N=1, seed=0):
    rng = np.random.default_rng(seed)
    B = int(np.prod(grid))
    return rng.uniform(-2, 2, (N, B, 3)).astype(F32), rng.uniform(0.2, 0.9, (N, B)).astype(F32), rng.uniform(-1, 1, (N, 3)).astype(F32)


def test_each_inlier_criterion():
    s, pk, base = _table((1, 1, 6))
    base[:] = 0
    pk[0, 0], pk[0, 1] = 0.05, np.nan
    s[0, 2, 1], s[0, 3, 0], s[0, 4, 2] = np.inf, np.nan, 5.0
    assert RB.inliers(s, pk, base).tolist() == [[True, False, False, False, True, True]], "no thresholds: finite peak and shift"
    assert RB.inliers(s, pk, base, min_peak=0.1).tolist() == [[False, False, False, False, True, True]]
    assert RB.inliers(s, pk, base, max_dev=(3, 3, 3)).tolist() == [[True, False, False, False, False, True]]
    pk[0, 5] = F32(0.7)                                                    # 0.699999988..: below the float64 0.7
    assert RB.inliers(s, pk, base, min_peak=float(F32(0.7)))[0, 5] and not RB.inliers(s, pk, base, min_peak=0.7)[0, 5], "float64 on the fp32 value"
    s[0, 5] = (1.0, -2.0, 0.5)
    assert RB.inliers(s, pk, base, max_dev=(1.0, 2.0, 0.5))[0, 5] and not RB.inliers(s, pk, base, max_dev=(1.0, 1.999, 0.5))[0, 5], "per component, <="
    pk[0, 4] = np.inf
    assert not RB.inliers(s, pk, base)[0, 4], "an infinite peak is no measurement"


def test_an_inlier_keeps_its_bits_and_an_outlier_takes_the_mean_of_its_inlier_neighbours():
    grid = (3, 3, 3)
    s, pk, base = _table(grid, seed=1)
    pk[0, 13] = np.nan                                                     # the centre: 26 neighbours
    field, ok = RB.field_fill(s, pk, base, grid)
    assert ok.sum() == 26 and not ok[0, 13]
    keep = np.arange(27) != 13
    assert np.array_equal(u32(field[0, keep]), u32(s[0, keep]))
    total = np.zeros(3)
    for b in range(27):                                                    # row-major, z slowest, the centre skipped
        if b != 13:
            total = total + s[0, b].astype(np.float64)
    assert np.array_equal(u32(field[0, 13]), u32((total / 26).astype(F32)))
    # the status is read from the input: two outliers side by side do not feed each other
    pk[0, 14] = np.nan
    field2, ok2 = RB.field_fill(s, pk, base, grid)
    total = sum((s[0, b].astype(np.float64) for b in range(27) if b not in (13, 14)), np.zeros(3))
    assert np.array_equal(u32(field2[0, 13]), u32((total / 25).astype(F32))) and ok2.sum() == 25


def test_neighbour_order_is_row_major_z_slowest():
    # neighbours whose float64 sum depends on the order
    grid = (3, 3, 1)
    s, pk, base = _table(grid, seed=2)
    s[0, :, 0] = [F32(1e17), 1.0, F32(-1e17), 1.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    pk[0, 4] = -1.0
    field, _ = RB.field_fill(s, pk, base, grid, min_peak=0.0)
    total = 0.0
    for b in (0, 1, 2, 3, 5, 6, 7, 8):
        total = total + float(s[0, b, 0])
    assert total == 5.0 and field[0, 4, 0] == F32(5.0 / 8), "(1e17 + 1) - 1e17 loses the 1 in this order and in no sorted one"


def test_a_corner_node_and_the_fallback_to_the_base():
    grid = (2, 3, 2)
    s, pk, base = _table(grid, N=2, seed=3)
    pk[0, 0] = np.nan                                                      # corner (0, 0, 0): neighbours 1, 2, 3 within z = 0 and 6, 7, 8, 9 above
    field, ok = RB.field_fill(s, pk, base, grid)
    nb = [1, 2, 3, 6, 7, 8, 9]
    total = sum((s[0, b].astype(np.float64) for b in nb), np.zeros(3))
    assert np.array_equal(u32(field[0, 0]), u32((total / 7).astype(F32)))
    assert np.array_equal(u32(field[1]), u32(s[1])) and ok[1].all(), "volumes are independent"
    pk[1, :] = np.nan                                                      # nothing to average: the base
    field, ok = RB.field_fill(s, pk, base, grid)
    assert not ok[1].any() and np.array_equal(u32(field[1]), u32(np.tile(base[1], (12, 1))))
    s2, pk2, base2 = _table((1, 1, 1), seed=4)
    s2[0, 0, 1] = np.nan
    field, ok = RB.field_fill(s2, pk2, base2, (1, 1, 1))
    assert not ok.any() and np.array_equal(u32(field[0, 0]), u32(base2[0])), "a grid of one node has no neighbour"


def test_nan_shifts_and_nan_peaks_never_reach_the_field():
    grid = (2, 2, 3)
    s, pk, base = _table(grid, seed=5)
    s[0, 1, 2], s[0, 4] = np.nan, np.inf
    pk[0, 7], pk[0, 10] = np.nan, -np.inf
    field, ok = RB.field_fill(s, pk, base, grid)
    assert np.isfinite(field).all() and ok[0].tolist() == [1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1]


# ------------------------------------------------------------------------------------------------ the warp
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_a_constant_field_is_the_rigid_shift_bit_for_bit(mode):
    rng = np.random.default_rng(6)
    x = rng.standard_normal((3, 5, 9, 11)).astype(F32)
    x[1, 2, 3, 4], x[2, 0, 0, 0] = np.nan, np.inf
    vec = np.array([[0.25, -1.5, 2.75], [1.0, -2.0, 3.0], [-1e-9, 0.5, -0.5]], dtype=F32)
    for grid, block in (((1, 1, 1), (5, 9, 11)), ((2, 3, 2), (3, 4, 6)), ((1, 2, 4), (5, 3, 2))):
        G = RB.block_grid(x.shape[1:], block, grid)
        field = np.tile(vec[:, None, :], (1, int(np.prod(grid)), 1))
        got, want = RB.warp(x, field, G, mode, fill=-3.0), R3.shift(x, vec, mode, fill=-3.0)
        assert np.array_equal(u32(got), u32(want)), (grid, mode)
    big = np.array([[5.0, 0.0, 0.0], [0.0, np.nan, 0.0], [1e30, -1e30, 0.0]], dtype=F32)
    G = RB.block_grid(x.shape[1:], (3, 4, 6), (2, 3, 2))
    got = RB.warp(x, np.tile(big[:, None, :], (1, 12, 1)), G, mode, fill=7.0)
    assert np.array_equal(u32(got), u32(R3.shift(x, big, mode, fill=7.0))) and (got == 7.0).all()


def test_an_integer_region_copies_bits_and_a_bad_node_fills_only_its_reach():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, 4, 12, 16)).astype(F32)
    G = RB.block_grid((4, 12, 16), (4, 4, 4), (1, 3, 4))
    field = np.zeros((1, 12, 3), dtype=F32)
    field[0, :, 2] = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, np.nan]           # dx = 1 everywhere but the last node
    out = RB.warp(x, field, G, fill=9.0)[0]
    assert np.array_equal(u32(out[:, :, :10]), u32(x[0, :, :, 1:11])), "columns up to centre 9.5 of the third node column see equal nodes"
    assert np.array_equal(u32(out[:, :6, :15]), u32(x[0, :, :6, 1:16])), "rows up to centre 5.5 of the second node row never reach the bad node"
    assert (out[:, 6:, 10:] == 9.0).all(), "every voxel that interpolates from the NaN node is filled"
    field[0, 11, 2] = 1e30
    out = RB.warp(x, field, G, fill=9.0)[0]
    assert (out[:, 6:, 10:] == 9.0).all() and np.array_equal(u32(out[:, :6, :15]), u32(x[0, :, :6, 1:16]))


# ------------------------------------------------------------------------------------------------ scene (P)
@pytest.mark.parametrize("shape,grid", P_CASES)
def test_planted_block_displacements_are_recovered_exactly(shape, grid):
    worst = 0.0
    m = tuple(v + 1 for v in P_MAX_D)
    for seed in P_SEEDS:
        sc = RB.scene_p(seed, shape, P_BLOCK, grid, max_d=P_MAX_D)
        B = int(np.prod(grid))
        assert sc.volumes.shape == (6,) + shape and sc.table.shape == (6, B, 3) and len({tuple(r) for r in sc.table[1]}) > 1
        c = RB.block_correlate(sc.volumes, sc.template, sc.grid, P_TAPER)
        s, ip, pk = R3.peak(c.reshape(6 * B, *P_BLOCK), m, subpixel=False)
        assert np.array_equal(s.reshape(6, B, 3), sc.table), (shape, seed)
        cc = c.reshape(6 * B, *P_BLOCK)
        for k in range(6 * B):
            mm = cc[k].copy()
            for a in (-1, 0, 1):
                for b in (-1, 0, 1):
                    for e in (-1, 0, 1):
                        mm[(ip[k, 0] + a) % P_BLOCK[0], (ip[k, 1] + b) % P_BLOCK[1], (ip[k, 2] + e) % P_BLOCK[2]] = -np.inf
            ratio = float(mm.max() / pk[k])
            worst = max(worst, ratio)
            assert ratio <= CAP, f"{shape}, seed {seed}, block {k}: second peak / peak = {ratio:.3f}"
        s2, pk2 = RB.block_shifts(sc.volumes, sc.template, sc.grid, m, P_TAPER, subpixel=False)
        field, ok = RB.field_fill(s2, pk2, np.zeros((6, 3), dtype=F32), grid)
        assert ok.all() and np.array_equal(field, sc.table)
    print(f"{shape} grid {grid}: largest second peak / peak = {worst:.3f}")


def test_a_uniform_table_is_an_exact_crop_of_the_still_scene():
    sc = RB.scene_p(0, (12, 48, 56), P_BLOCK, (1, 2, 2), max_d=P_MAX_D, uniform=True)
    assert (sc.table == sc.table[:, :1]).all() and sc.table[1:].any()
    reg = RB.warp(sc.volumes, sc.table, sc.grid, mode="nearest")
    z0, z1, y0, y1, x0, x1 = R3.valid_box(sc.table.reshape(-1, 3), (12, 48, 56))
    assert z1 - z0 >= 8 and np.array_equal(u32(reg[:, z0:z1, y0:y1, x0:x1]), u32(sc.still[:, z0:z1, y0:y1, x0:x1]))


# ------------------------------------------------------------------------------------------------ the entry points' arguments
def test_reg_window_blocks3d_arguments(L, ptr):
    x, wz, wy, wx, out = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(5))
    I = ctypes.c_int32

    def call(x=x, N=2, D=3, H=4, W=8, vs=96, o=(0, 1, 0, 2, 0, 2, 4), g=(2, 2, 3), b=(2, 2, 4), wz=wz, wy=wy, wx=wx, out=out, null_o=False):
        return L.cwfa_reg_window_blocks3d_f32(x, N, D, H, W, vs, None if null_o else (I * len(o))(*o), *g, *b, wz, wy, wx, out, None)

    for k in ("x", "wz", "wy", "wx", "out"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_window_blocks3d_f32: null" in L.cwfa_last_error()
    assert call(null_o=True) == -1 and b"null" in L.cwfa_last_error()
    assert call(N=-1) == -2 and call(D=-3) == -2 and b"negative" in L.cwfa_last_error()
    assert call(D=1 << 10, H=1 << 11, W=1 << 10) == -2 and b"too large" in L.cwfa_last_error()
    for g in ((0, 2, 3), (2, -1, 3), (2, 2, 0), (17, 16, 16), (1 << 20, 1 << 20, 1)):
        assert call(g=g) == -2 and b"grid" in L.cwfa_last_error(), g
    for b in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (4, 2, 4), (2, 5, 4), (2, 2, 9), (-1, 2, 4)):
        assert call(b=b) == -2 and b"block" in L.cwfa_last_error(), b
    for o in ((-1, 1, 0, 2, 0, 2, 4), (0, 2, 0, 2, 0, 2, 4), (0, 1, 0, 3, 0, 2, 4), (0, 1, 0, 2, 0, 2, 5), (0, 1, 0, 2, -4, 2, 4)):
        assert call(o=o) == -1 and b"outside the volume" in L.cwfa_last_error(), o
    for k in ("x", "wz", "wy", "wx", "out"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 16384 + 2)}) == -3 and b"4-byte" in L.cwfa_last_error(), k
    assert call(vs=95) == -1 and call(vs=-96) == -1 and b"stride" in L.cwfa_last_error()
    assert call(out=x) == -1 and b"must not" in L.cwfa_last_error()
    assert call(N=0) == 0, "empty: no launch"
    assert call(D=0, vs=0) == -2 and call(W=0, vs=0) == -2, "a block of at least one voxel does not fit an empty volume"


def test_reg_field_fill_arguments(L, ptr):
    s, pk, base, field, inl = (ctypes.c_void_p(ptr.value + 2048 * k) for k in range(5))
    D3 = ctypes.c_double * 3

    def call(s=s, pk=pk, base=base, N=2, g=(2, 2, 3), min_peak=0.1, md=(1.0, 2.0, 2.0), field=field, inl=inl):
        return L.cwfa_reg_field_fill(s, pk, base, N, *g, min_peak, None if md is None else D3(*md), field, inl, None)

    for k in ("s", "pk", "base", "field", "inl"):
        assert call(**{k: None}) == -1 and b"cwfa_reg_field_fill: null" in L.cwfa_last_error()
    assert call(N=-1) == -2 and b"negative" in L.cwfa_last_error()
    for g in ((0, 2, 3), (2, -1, 3), (2, 2, 0), (17, 16, 16), (1 << 20, 1 << 20, 1)):
        assert call(g=g) == -2 and b"grid" in L.cwfa_last_error(), g
    assert call(min_peak=float("nan")) == -1 and b"min_peak" in L.cwfa_last_error()
    for md in ((-1.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, -0.5)):
        assert call(md=md) == -1 and b"max_dev" in L.cwfa_last_error(), md
    for k in ("s", "pk", "base", "field"):
        assert call(**{k: ctypes.c_void_p(ptr.value + 16384 + 2)}) == -3 and b"4-byte" in L.cwfa_last_error(), k
    assert call(field=s) == -1 and b"must not be the shift table" in L.cwfa_last_error()
    assert call(N=0) == 0 and call(N=0, md=None) == 0, "empty: no launch"


def test_reg_warp3d_arguments(L, ptr):
    x, field, iz, tz, iy, ty, ix, tx, out = (ctypes.c_void_p(ptr.value + 1024 * k) for k in range(9))

    def call(x=x, N=2, D=3, H=4, W=8, vs=96, field=field, g=(2, 2, 3), iz=iz, tz=tz, iy=iy, ty=ty, ix=ix, tx=tx, mode=0, fill=0.0, out=out):
        return L.cwfa_reg_warp3d_f32(x, N, D, H, W, vs, field, *g, iz, tz, iy, ty, ix, tx, mode, fill, out, None)

    names = ("x", "field", "iz", "tz", "iy", "ty", "ix", "tx", "out")
    for k in names:
        assert call(**{k: None}) == -1 and b"cwfa_reg_warp3d_f32: null" in L.cwfa_last_error()
    assert call(mode=2) == -1 and call(mode=-1) == -1 and b"mode" in L.cwfa_last_error()
    assert call(N=-1) == -2 and call(D=-1) == -2 and call(H=-1) == -2 and call(W=-1) == -2 and b"negative" in L.cwfa_last_error()
    assert call(D=1 << 10, H=1 << 11, W=1 << 10) == -2 and call(W=1 << 30, D=1, H=1) == -2 and b"too large" in L.cwfa_last_error()
    for g in ((0, 2, 3), (2, -1, 3), (2, 2, 0), (17, 16, 16), (1 << 20, 1 << 20, 1)):
        assert call(g=g) == -2 and b"grid" in L.cwfa_last_error(), g
    for k in names:
        assert call(**{k: ctypes.c_void_p(ptr.value + 16384 + 2)}) == -3 and b"4-byte" in L.cwfa_last_error(), k
    assert call(vs=95) == -1 and call(vs=-97) == -1 and b"stride" in L.cwfa_last_error()
    assert call(out=x) == -1 and b"alias" in L.cwfa_last_error()
    assert call(N=0) == 0 and call(D=0, vs=0) == 0 and call(H=0, vs=0) == 0 and call(W=0, vs=0) == 0, "empty: no launch"


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_python_layer_refuses_before_any_device_work():
    from cwfa_amd import ops
    from cwfa_amd.CWFA import (PiecewiseVolumeRegistrar, block_grid, estimate_block_shifts, register_volumes_piecewise, warp_volumes)
    v, t = torch.zeros(4, 6, 40, 48), torch.zeros(6, 40, 48)
    G = block_grid((6, 40, 48), (6, 20, 24))
    assert G.grid == (1, 2, 2) and G.block == (6, 20, 24)
    f = torch.zeros(4, 1, 2, 2, 3)
    for bad in ((6, 40), "x", (0, 40, 48), (6.5, 40, 48)):
        with pytest.raises(ValueError, match="shape"):
            block_grid(bad)
    for bad in ((6, 20), (0, 20, 24), (6, -1, 24)):
        with pytest.raises(ValueError, match="block"):
            block_grid((6, 40, 48), bad)
    for bad in ((1, 2), (0, 2, 2), (1, 2, 2.5), (17, 16, 16)):
        with pytest.raises(ValueError, match="grid"):
            block_grid((6, 40, 48), (6, 20, 24), bad)
    for call in (lambda: estimate_block_shifts(v[..., ::2], t[..., ::2], G), lambda: register_volumes_piecewise(v[:, :, ::2]), lambda: warp_volumes(v[..., ::2], f, G),
                 lambda: estimate_block_shifts(v[0], t, G), lambda: register_volumes_piecewise(v[0]), lambda: warp_volumes(v[0], f, G)):
        with pytest.raises(ValueError, match=r"contiguous \[N,D,H,W\]"):
            call()
    for call in (lambda: estimate_block_shifts(v.half(), t, G), lambda: register_volumes_piecewise(v.double(), t), lambda: warp_volumes(v.half(), f, G)):
        with pytest.raises(ValueError, match="float32 stack"):
            call()
    for bad in (torch.zeros(6, 40, 47), torch.zeros(6, 40, 48, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="template"):
            estimate_block_shifts(v, bad, G)
    for fn in (lambda **k: estimate_block_shifts(v, t, G, **k), lambda **k: register_volumes_piecewise(v, t, **k)):
        with pytest.raises(ValueError, match="'dft'.*not built"):
            fn(subpixel="dft")
        with pytest.raises(ValueError, match="min_peak"):
            fn(min_peak=float("nan"))
        for md in (-1.0, (1, 2), (1.0, float("nan"), 1.0), "x"):
            with pytest.raises(ValueError, match="max_dev"):
                fn(max_dev=md)
        with pytest.raises(ValueError, match="chunk"):
            fn(chunk=0)
    for bad in ((1, 2, 2), None, block_grid((6, 40, 50), (6, 20, 24))):
        with pytest.raises(ValueError, match="grid"):
            estimate_block_shifts(v, t, bad)
        with pytest.raises(ValueError, match="grid"):
            warp_volumes(v, f, bad)
    for m in ((3, 8, 8), (2, 10, 8), (2, 8, 12), (2, 8)):                  # against the BLOCK: 6 x 20 x 24
        with pytest.raises(ValueError, match="max_shift.*block"):
            estimate_block_shifts(v, t, G, max_shift=m)
    for tp in ((4, 0, 0), (0, 11, 0), (0, 0, 13)):
        with pytest.raises(ValueError, match="taper.*block"):
            estimate_block_shifts(v, t, G, taper=tp)
    for bad in (torch.zeros(3, 3), torch.zeros(4, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="base"):
            estimate_block_shifts(v, t, G, base=bad)
    for bad in (torch.zeros(4, 1, 2, 2, 2), torch.zeros(3, 1, 2, 2, 3), torch.zeros(4, 5, 3), torch.zeros(4, 4, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="field"):
            warp_volumes(v, bad, G)
    with pytest.raises(ValueError, match="mode"):
        warp_volumes(v, f, G, mode="cubic")
    for out in (v, v[:], v[1:]):
        with pytest.raises(ValueError, match="alias"):
            warp_volumes(v, f, G, out=out)
    with pytest.raises(ValueError, match="alias"):
        register_volumes_piecewise(v, t, out=v)
    with pytest.raises(ValueError, match="n_iter"):
        register_volumes_piecewise(v, t, n_iter=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PiecewiseVolumeRegistrar(t, G)
    w = [torch.zeros(n) for n in (6, 20, 24)]
    with pytest.raises(ValueError, match="outside the volume"):
        ops.reg_window_blocks3d(v, ([0], [0, 21], [0, 24]), (6, 20, 24), *w)
    with pytest.raises(ValueError, match="does not fit"):
        ops.reg_window_blocks3d(v, ([0], [0, 20], [0, 24]), (7, 20, 24), *w)
    with pytest.raises(ValueError, match="more than 4096"):
        ops.reg_window_blocks3d(v, ([0] * 17, [0] * 16, [0] * 16), (6, 20, 24), *w)
    with pytest.raises(ValueError, match="shifts"):
        ops.reg_field_fill(torch.zeros(4, 5, 3), torch.zeros(4, 4), torch.zeros(4, 3), (1, 2, 2))
    with pytest.raises(ValueError, match="tables"):
        ops.reg_warp3d(v, f.reshape(4, 4, 3), (1, 2, 2), (1, 2, 3))
    for call in (lambda: estimate_block_shifts(v, t, G), lambda: warp_volumes(v, f, G), lambda: register_volumes_piecewise(v, t),
                 lambda: ops.reg_window_blocks3d(v, G.origins, G.block, *w), lambda: ops.reg_field_fill(f.reshape(4, 4, 3), torch.zeros(4, 4), torch.zeros(4, 3), (1, 2, 2)),
                 lambda: ops.reg_warp3d(v, f.reshape(4, 4, 3), (1, 2, 2), tuple(torch.from_numpy(a) for a in RB.tables(RB.block_grid((6, 40, 48), (6, 20, 24)))))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_the_names_are_exported_and_the_valid_box_is_documented():
    from cwfa_amd import CWFA
    for name in ("block_grid", "BlockGrid", "estimate_block_shifts", "warp_volumes", "register_volumes_piecewise", "PiecewiseRegistration",
                 "PiecewiseVolumeRegistrar"):
        assert name in CWFA.__all__ and hasattr(CWFA, name)
    assert CWFA.PiecewiseRegistration._fields == ("volumes", "field", "peak", "inlier", "shifts", "template")
    assert "valid_box(field.reshape(-1, 3), shape)" in CWFA.warp_volumes.__doc__ and "convex combination" in CWFA.warp_volumes.__doc__
    # the bound itself, on the restatement: the interpolated vectors stay inside the nodes' range up to an ulp
    G = RB.block_grid((7, 20, 18), (3, 6, 5), (3, 4, 4))
    nodes = np.random.default_rng(8).uniform(-3, 3, (3, 4, 4, 3)).astype(F32)
    d = RB.field_at(nodes, RB.tables(G))
    lo, hi = nodes.reshape(-1, 3).min(0), nodes.reshape(-1, 3).max(0)
    assert (d >= lo - 1e-5).all() and (d <= hi + 1e-5).all()
