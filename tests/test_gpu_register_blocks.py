"""GPU: piecewise-rigid registration of volumes.  The three kernels bit for bit against the numpy restatement
tests/register_blocks_ref.py on the SAME handed-in inputs, at the smallest shapes that reach every path (one voxel, odd sizes on the
element path, the 16-byte path, a volume stride that is and is not a multiple of 4, a base that breaks 16-byte alignment, two and
three z segments of the warp, overlapping and gapped grids, one block along each axis in turn); a constant field against
``ops.reg_shift3d``; then the public functions end to end on the planted scenes: (P), where the planted table is recovered exactly and
a uniform one undone bit for bit, and (S), where the piecewise result must be closer to the still scene than the rigid one."""
import numpy as np
import pytest
import torch

import register3d_ref as R3
import register_blocks_ref as RB
from test_gpu_register import device_stack, same_bits, same_values

pytestmark = pytest.mark.gpu
F32 = np.float32
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

# (N, D, H, W, block, grid, unused elements behind every volume, elements in front of the first volume).  12 x 16 with bx = 8 or 4: the
# 16-byte forms; 10 x 13: element by element; 17 and 33 planes: two and three z segments of the warp (a segment holds at most 16);
# grids that overlap ((3, 4, 8) x (2, 3, 2) in 5 x 12 x 16 along z), leave gaps ((2, 3, 2) x (2, 3, 4) along y and x) and have one
# block along each axis in turn
LAYOUTS = [(1, 1, 1, 1, (1, 1, 1), (1, 1, 1), 0, 0), (3, 2, 5, 7, (2, 3, 3), (1, 2, 3), 0, 0), (2, 5, 12, 16, (3, 4, 8), (2, 3, 2), 0, 0),
           (2, 6, 10, 13, (2, 4, 5), (3, 3, 3), 0, 0), (2, 5, 12, 16, (3, 4, 8), (2, 3, 2), 8, 0), (2, 5, 12, 16, (3, 4, 8), (2, 3, 2), 3, 0),
           (2, 5, 12, 16, (2, 3, 4), (2, 3, 4), 0, 1), (2, 2, 5, 7, (2, 2, 2), (1, 3, 4), 2, 3), (1, 17, 4, 8, (5, 2, 4), (4, 2, 2), 0, 0),
           (2, 33, 3, 5, (9, 3, 2), (5, 1, 3), 1, 0), (2, 5, 12, 16, (5, 4, 4), (1, 3, 4), 0, 0), (2, 5, 12, 16, (2, 12, 4), (3, 1, 4), 0, 0),
           (2, 5, 12, 16, (2, 4, 16), (3, 3, 1), 0, 0)]


def volume_data(N, D, H, W, specials=False):
    rng = np.random.default_rng(29 + 1000 * N + 100 * D + 10 * H + W)
    x = (rng.standard_normal((N, D, H, W)) * 100.0 + 300.0).astype(F32)
    if specials and H >= 3 and W >= 4:
        z = min(1, D - 1)
        x[0, 0, 1, 2], x[0, z, 2, 3], x[N - 1, D - 1, H - 1, W - 1], x[0, 0, 0, 0], x[0, z, H - 1, 1] = np.nan, np.inf, -np.inf, -0.0, 0.0
    return x


def dev_tables(G):
    return tuple(dev(a) for a in RB.tables(G))


def unaligned_out(shape):
    """A contiguous device tensor of ``shape`` that starts 4 bytes behind a 16-byte boundary."""
    n = int(np.prod(shape))
    buf = torch.full((n + 1,), 7e4, dtype=torch.float32, device="cuda")
    out = buf[1:].view(shape)
    assert out.data_ptr() % 16 == 4
    return out


# ------------------------------------------------------------------------------------------------ the cut and the taper
@pytest.mark.parametrize("N,D,H,W,block,grid,pad,offset", LAYOUTS)
def test_window_blocks_bit_for_bit(N, D, H, W, block, grid, pad, offset):
    from cwfa_amd import ops
    x = volume_data(N, D, H, W)
    G = RB.block_grid((D, H, W), block, grid)
    wins = R3.tapers(block, tuple(min(2, b // 2) for b in block))
    want = RB.cut(x, G.origins, block, wins)
    B = int(np.prod(grid))
    got = ops.reg_window_blocks3d(device_stack(x, pad, offset), G.origins, block, *(dev(w) for w in wins))
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, B, *block) and same_bits(got, want)
    out = unaligned_out((N, B, *block))
    assert ops.reg_window_blocks3d(device_stack(x, pad, offset), [o.tolist() for o in G.origins], block, *(dev(w) for w in wins), out=out) is out
    assert same_bits(out, want), "an out that breaks 16-byte alignment: the element path"
    ones = ops.reg_window_blocks3d(device_stack(x, pad, offset), G.origins, block, *(torch.ones(b, device="cuda") for b in block))
    for n in (0, N - 1):
        for b, (oz, oy, ox) in enumerate((oz, oy, ox) for oz in G.origins[0] for oy in G.origins[1] for ox in G.origins[2]):
            assert same_bits(ones[n, b], x[n, oz:oz + block[0], oy:oy + block[1], ox:ox + block[2]]), "taper 0: the block itself"


def test_window_blocks_take_any_origin_inside_the_volume_and_walk_the_volumes():
    from cwfa_amd import ops
    x = volume_data(2, 4, 9, 21)
    origins, block = ([2, 0, 1], [5, 0], [13, 1, 7, 2]), (2, 4, 8)         # unsorted, unaligned, touching the far faces
    wins = R3.tapers(block, (1, 2, 3))
    assert same_bits(ops.reg_window_blocks3d(dev(x), origins, block, *(dev(w) for w in wins)), RB.cut(x, origins, block, wins))
    many = np.random.default_rng(1).standard_normal((70000, 1, 1, 4)).astype(F32)   # more volumes than a grid axis holds
    w1 = [np.ones(1, dtype=F32), np.ones(1, dtype=F32), np.array([0.5, 1.0], dtype=F32)]
    got = ops.reg_window_blocks3d(dev(many), ([0], [0], [0, 2]), (1, 1, 2), *(dev(w) for w in w1))
    assert same_bits(got, RB.cut(many, ([0], [0], [0, 2]), (1, 1, 2), w1))


# ------------------------------------------------------------------------------------------------ the clean-up
@pytest.mark.parametrize("grid", [(1, 1, 1), (3, 4, 5), (1, 5, 1), (2, 2, 2), (4, 1, 3)])
def test_field_fill_against_the_restatement(grid):
    from cwfa_amd import ops
    rng = np.random.default_rng(41 + sum(grid))
    N, B = 4, int(np.prod(grid))
    s = rng.uniform(-3, 3, (N, B, 3)).astype(F32)
    pk = rng.uniform(0.05, 0.9, (N, B)).astype(F32)
    base = rng.uniform(-1, 1, (N, 3)).astype(F32)
    gz, gy, gx = grid
    node = lambda z, y, x: (z * gy + y) * gx + x
    planted = [node(0, 0, 0), node(gz - 1, gy - 1, gx - 1), node(0, gy - 1, 0), node(0, gy // 2, 0), node(gz // 2, gy // 2, gx // 2), node(gz // 2, gy // 2, min(gx - 1, gx // 2 + 1))]
    for k, b in enumerate(planted):                                        # corners, an edge, the interior and its neighbour
        if k % 3 == 0:
            pk[0, b] = np.nan
        elif k % 3 == 1:
            s[0, b, k % 3] = np.inf
        else:
            s[0, b] += 50.0
        pk[1, b] = 0.01
    s[2, :, 0] = np.nan                                                    # volume 2: nothing to average, the base
    s[3, ::2, 1] *= F32(1e17)                                              # volume 3: sums whose order shows
    pk[3, 1::2] = -np.inf
    for min_peak, max_dev in ((0.0, None), (0.04, (4.0, 4.0, 4.0)), (0.3, (2.0, 1.0, 0.5)), (2.0, None)):
        want_f, want_i = RB.field_fill(s, pk, base, grid, min_peak, max_dev)
        field, inlier = ops.reg_field_fill(dev(s), dev(pk), dev(base), grid, min_peak, max_dev)
        assert inlier.dtype == torch.uint8 and np.array_equal(inlier.cpu().numpy(), want_i), (min_peak, max_dev)
        assert same_bits(field, want_f), (min_peak, max_dev)
    again = ops.reg_field_fill(dev(s), dev(pk), dev(base), grid, 0.04, (4.0, 4.0, 4.0))
    assert same_bits(again[0], RB.field_fill(s, pk, base, grid, 0.04, (4.0, 4.0, 4.0))[0]), "bitwise repeatable"


# ------------------------------------------------------------------------------------------------ the warp
def node_fields(kind, N, D, H, W, grid, rng):
    B = int(np.prod(grid))
    if kind == "constant":
        return np.tile(rng.uniform(-2.5, 2.5, (N, 1, 3)).astype(F32), (1, B, 1))
    if kind == "integer":
        return rng.integers(-2, 3, (N, B, 3)).astype(F32)
    if kind == "fractional":
        return rng.uniform(-1.5, 1.5, (N, B, 3)).astype(F32)
    if kind == "steep":                                                   # floor boundaries inside one thread's four voxels
        return (rng.uniform(-1.0, 1.0, (N, B, 3)) * np.array([D, H, W])).astype(F32)
    if kind == "far":                                                     # displacements at and beyond the side
        f = rng.uniform(-0.5, 0.5, (N, B, 3)).astype(F32)
        f[:, ::2] += np.array([D, -H, W + 1], dtype=F32)
        return f
    f = rng.uniform(-1.5, 1.5, (N, B, 3)).astype(F32)                     # "bad": one node each of +1e30, -1e30 and NaN
    f[0, 0, 2], f[N - 1, B - 1, 0], f[0, B // 2, 1] = 1e30, -1e30, np.nan
    return f


@pytest.mark.parametrize("N,D,H,W,block,grid,pad,offset", LAYOUTS)
def test_warp_bit_for_bit(N, D, H, W, block, grid, pad, offset):
    from cwfa_amd import ops
    x = volume_data(N, D, H, W)
    G = RB.block_grid((D, H, W), block, grid)
    tabs = dev_tables(G)
    rng = np.random.default_rng(53 + D + H + W)
    for k, kind in enumerate(("constant", "integer", "fractional", "steep", "far", "bad")):
        field = node_fields(kind, N, D, H, W, grid, rng)
        for mode in ("bilinear", "nearest"):
            fill = (0.0, -7.5)[(k + (mode == "nearest")) % 2]
            want = RB.warp(x, field, G, mode, fill)
            got = ops.reg_warp3d(device_stack(x, pad, offset), dev(field), grid, tabs, mode=mode, fill=fill)
            assert got.dtype == torch.float32 and same_bits(got, want), (kind, mode)
            if kind in ("fractional", "bad"):
                out = unaligned_out((N, D, H, W))
                assert ops.reg_warp3d(device_stack(x, pad, offset), dev(field), grid, tabs, mode=mode, fill=fill, out=out) is out
                assert same_bits(out, want), (kind, mode, "an out that breaks 16-byte alignment: one voxel per thread")


@pytest.mark.parametrize("N,D,H,W,block,grid,pad,offset", [LAYOUTS[k] for k in (0, 2, 3, 5, 8, 9)])
def test_a_constant_field_is_reg_shift3d_bit_for_bit(N, D, H, W, block, grid, pad, offset):
    from cwfa_amd import ops
    G = RB.block_grid((D, H, W), block, grid)
    tabs, B = dev_tables(G), int(np.prod(grid))
    rng = np.random.default_rng(61 + D + H + W)
    x = volume_data(N, D, H, W)
    for vec in (rng.uniform(-2.5, 2.5, (N, 3)), rng.integers(-2, 3, (N, 3)), np.array([[-1e-9, 0.5, -0.5]] * N), np.array([[D, 0.25, 0.0]] * N),
                np.array([[0.0, np.nan, 0.0]] * N), np.array([[1e30, -1e30, 0.5]] * N)):
        vec = vec.astype(F32)
        field = dev(np.tile(vec[:, None, :], (1, B, 1)))
        for mode in ("bilinear", "nearest"):
            want = ops.reg_shift3d(device_stack(x, pad, offset), dev(vec), mode=mode, fill=2.5)
            assert torch.equal(ops.reg_warp3d(device_stack(x, pad, offset), field, grid, tabs, mode=mode, fill=2.5).view(torch.int32), want.view(torch.int32))
    special = volume_data(N, D, H, W, specials=True)                       # NaN, +-inf, -0.0 in the volumes: an integer vector copies their bits
    vec = np.tile(np.array([[min(1, D - 1), -1.0, 1.0]], dtype=F32), (N, 1))
    want = ops.reg_shift3d(dev(special), dev(vec), fill=2.5)
    got = ops.reg_warp3d(dev(special), dev(np.tile(vec[:, None, :], (1, B, 1))), grid, tabs, fill=2.5)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and same_bits(got, R3.shift(special, vec, fill=2.5))


def test_one_block_is_the_rigid_resampling_and_the_public_warp_takes_the_five_axis_field():
    from cwfa_amd.CWFA import block_grid, shift_volumes, warp_volumes
    x = volume_data(3, 6, 10, 12)
    G = block_grid((6, 10, 12), (32, 128, 128))
    assert G.grid == (1, 1, 1) and G.block == (6, 10, 12)
    vec = np.random.default_rng(3).uniform(-2, 2, (3, 3)).astype(F32)
    want = shift_volumes(dev(x), dev(vec), fill=1.0)
    assert torch.equal(warp_volumes(dev(x), dev(vec).view(3, 1, 1, 1, 3), G, fill=1.0).view(torch.int32), want.view(torch.int32))
    assert torch.equal(warp_volumes(dev(x), dev(vec).view(3, 1, 3), G, fill=1.0).view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------------ scene (P), end to end
P_SHAPE, P_BLOCK, P_GRID = (12, 48, 56), (12, 24, 28), (1, 2, 2)
KW = dict(max_shift=(3, 4, 4), taper=(1, 3, 3))


@pytest.mark.parametrize("seed", [0, 1])
def test_the_planted_table_is_recovered_exactly(seed):
    from cwfa_amd.CWFA import block_grid, estimate_block_shifts
    sc = RB.scene_p(seed, P_SHAPE, P_BLOCK, P_GRID)
    G = block_grid(P_SHAPE, P_BLOCK, P_GRID, device="cuda")
    field, peak, inlier = estimate_block_shifts(dev(sc.volumes), dev(sc.template), G, subpixel=False, **KW)
    assert tuple(field.shape) == (6, 1, 2, 2, 3) and tuple(peak.shape) == (6, 1, 2, 2) and tuple(inlier.shape) == (6, 1, 2, 2) and inlier.dtype == torch.uint8
    assert np.array_equal(field.cpu().numpy().reshape(6, 4, 3), sc.table), "exactly the planted table"
    assert bool(inlier.all()) and float(peak.min()) > 0.1
    chunked = estimate_block_shifts(dev(sc.volumes), dev(sc.template), G, subpixel=False, chunk=4, **KW)
    assert same_bits(chunked[0], field.cpu().numpy()) and same_bits(chunked[1], peak.cpu().numpy()), "any chunking"
    # a block whose estimate is thrown out takes its neighbours' mean: with max_dev = 0 around a base nobody has, every node is the base
    base = torch.full((6, 3), 0.5, device="cuda")
    f2, _, in2 = estimate_block_shifts(dev(sc.volumes), dev(sc.template), G, subpixel=False, max_dev=0.0, base=base, **KW)
    assert not bool(in2.any()) and bool((f2 == 0.5).all())


@pytest.mark.parametrize("seed", [0, 1])
def test_a_uniform_table_is_undone_bit_for_bit_and_the_activity_map_is_the_still_scene(seed):
    from cwfa_amd.CWFA import ActivityMap, PiecewiseVolumeRegistrar, block_grid, register_volumes_piecewise, valid_box
    sc = RB.scene_p(seed, P_SHAPE, P_BLOCK, P_GRID, uniform=True)
    volumes, still, template = dev(sc.volumes), dev(sc.still), dev(sc.template)
    reg = register_volumes_piecewise(volumes, template, grid=P_GRID, block=P_BLOCK, subpixel=False, mode="nearest", **KW)
    assert np.array_equal(reg.field.cpu().numpy().reshape(6, 4, 3), sc.table) and same_bits(reg.shifts, reg.field.cpu().numpy()) and reg.template is template
    z0, z1, y0, y1, x0, x1 = box = valid_box(reg.field.reshape(-1, 3), P_SHAPE)
    assert box == R3.valid_box(sc.table.reshape(-1, 3), P_SHAPE) and z1 - z0 >= 8 and y1 - y0 >= 42 and x1 - x0 >= 50
    crop = lambda t: t[..., z0:z1, y0:y1, x0:x1].contiguous()
    assert same_bits(crop(reg.volumes), sc.still[:, z0:z1, y0:y1, x0:x1]), "the registered stack is the still scene"
    registrar = PiecewiseVolumeRegistrar(template, block_grid(P_SHAPE, P_BLOCK, P_GRID), mode="nearest", subpixel=False, **KW)
    a, b, moved = (ActivityMap(P_SHAPE, "cuda") for _ in range(3))
    for s, e in ((0, 4), (4, 6)):                                           # the series in two chunks, never resident
        a.update(registrar(volumes[s:e]))
    assert len(registrar.field) == 2 and same_bits(registrar.all_fields(), reg.field.cpu().numpy()) and same_bits(registrar.all_peaks(), reg.peak.cpu().numpy())
    b.update(still)
    moved.update(volumes)
    sa, sb, sm = (crop(m.finish("std")[0]) for m in (a, b, moved))
    assert same_bits(sa, sb.cpu().numpy()), "the activity map of the registered series is the still scene's on the box"
    assert not same_bits(sm, sb.cpu().numpy()), "the unregistered series' is not"
    one = registrar(volumes[5])
    assert tuple(one.shape) == P_SHAPE and same_bits(one, reg.volumes[5].cpu().numpy()), "one volume"


# ------------------------------------------------------------------------------------------------ scene (S): the feature's purpose
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_piecewise_is_closer_to_the_still_scene_than_rigid(seed):
    from cwfa_amd.CWFA import register_volumes, register_volumes_piecewise, valid_box
    sc = RB.scene_s(seed, P_SHAPE, P_BLOCK, P_GRID)
    volumes, template = dev(sc.volumes), dev(sc.template)
    pw = register_volumes_piecewise(volumes, template, grid=P_GRID, block=P_BLOCK, **KW)
    rg = register_volumes(volumes, template, **KW)
    both = torch.cat((pw.field.reshape(-1, 3), rg.shifts))
    box = valid_box(both, P_SHAPE)
    assert box[1] - box[0] >= 6 and box[3] - box[2] >= 36 and box[5] - box[4] >= 44
    e_pw = RB.valid_mean_abs(pw.volumes.cpu().numpy(), sc.still, box)
    e_rg = RB.valid_mean_abs(rg.volumes.cpu().numpy(), sc.still, box)
    e_raw = RB.valid_mean_abs(sc.volumes, sc.still, box)
    print(f"seed {seed}: mean |registered - still| on the valid box: piecewise {e_pw:.3f}, rigid {e_rg:.3f}, unregistered {e_raw:.3f}; "
          f"piecewise / rigid = {e_pw / e_rg:.3f}")
    assert e_pw < e_rg, "a field that differs per block is what the rigid vector cannot follow"


# ------------------------------------------------------------------------------------------------ sub-voxel block shifts
# The largest |device - restatement| of the sub-voxel block shifts of scene (S) over seeds 0 .. 2, observed on the MI355X: 1.967e-06
# voxels (section 30.4 saw 2.4e-07 on whole volumes: a block's correlation peak is flatter on this scene, whose displacement varies
# inside a block).  The two differ only in the transforms (rocFFT in fp32 against numpy.fft in float64), whose rounding reaches the
# shift through the parabola's denominator.  The bound is 4 x the observation, the margin section 26.4 uses for that.
OBSERVED_SUBVOXEL_DIFF = 1.967e-06
SUBVOXEL_DIFF_BOUND = 4.0 * OBSERVED_SUBVOXEL_DIFF


def test_subvoxel_block_shifts_against_the_restatement():
    from cwfa_amd.CWFA import block_grid, estimate_block_shifts
    worst = 0.0
    G = block_grid(P_SHAPE, P_BLOCK, P_GRID)
    for seed in (0, 1, 2):
        sc = RB.scene_s(seed, P_SHAPE, P_BLOCK, P_GRID)
        c = RB.block_correlate(sc.volumes, sc.template, sc.grid, KW["taper"])
        want, wi, wpk = R3.peak(c.reshape(24, *P_BLOCK), KW["max_shift"], True)
        field, pk, inlier = estimate_block_shifts(dev(sc.volumes), dev(sc.template), G, base=torch.zeros(6, 3, device="cuda"), chunk=2, **KW)
        got = field.cpu().numpy().reshape(24, 3)
        assert bool(inlier.all())
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.all(np.abs(got - wi) <= 0.5), "the same integer peak: the refinement moves it by at most half a voxel"
        assert float(np.abs(pk.cpu().numpy().reshape(24) - wpk).max()) < 1e-3
    print(f"largest |device - restatement| of the sub-voxel block shifts = {worst:.3e} voxels")
    assert worst <= SUBVOXEL_DIFF_BOUND
