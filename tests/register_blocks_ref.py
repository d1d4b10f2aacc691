"""The numpy restatement of the piecewise-rigid registration of volumes and the planted scenes of its tests.

The restatements of sections 26 and 30 (tests/register_ref.py, tests/register3d_ref.py) supply the taper, the correlation, the peak
and the rigid resampling; this file adds the grid of blocks, the cut, the clean-up of the shift table, the interpolation of the
field and the resampling under a displacement per voxel, one rounding at a time."""
from collections import namedtuple

import numpy as np

import register3d_ref as R3
import register_ref as R

F32 = np.float32
Grid = namedtuple("Grid", ["shape", "block", "grid", "origins", "centers", "idx", "t"])


# ------------------------------------------------------------------------------------------------ step 1: the grid
def axis_grid(S, b, g):
    """(origins int [g], centres float64 [g], idx int32 [S], t float32 [S]) of one axis, written out coordinate by coordinate."""
    o = [(i * (S - b)) // (g - 1) for i in range(g)] if g > 1 else [(S - b) // 2]
    c = [float(v) + (b - 1) / 2.0 for v in o]
    idx, t = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=F32)
    for p in range(S):
        if g == 1 or p <= c[0]:
            continue
        if p >= c[g - 1]:
            idx[p] = g - 1
            continue
        i = max(k for k in range(g) if c[k] <= p)
        idx[p], t[p] = i, F32((p - c[i]) / (c[i + 1] - c[i]))
    return np.array(o, dtype=np.int32), np.array(c, dtype=np.float64), idx, t


def block_grid(shape, block, grid=None):
    block = tuple(min(int(b), int(s)) for b, s in zip(block, shape))
    grid = tuple(-(-s // b) for s, b in zip(shape, block)) if grid is None else tuple(grid)
    axes = [axis_grid(S, b, g) for S, b, g in zip(shape, block, grid)]
    return Grid(tuple(shape), block, grid, *(tuple(a[k] for a in axes) for k in range(4)))


def tables(G):
    return tuple(a for pair in zip(G.idx, G.t) for a in pair)


# ------------------------------------------------------------------------------------------------ step 2: the cut and the taper
def cut(x, origins, block, wins):
    """fp32 [N, B, bz, by, bx]: every block of every volume, windowed as register3d_ref.window windows a volume."""
    bz, by, bx = block
    out = [[R3.window(v[oz:oz + bz, oy:oy + by, ox:ox + bx], *wins) for oz in origins[0] for oy in origins[1] for ox in origins[2]] for v in x]
    return np.array(out, dtype=F32).reshape(len(x), len(origins[0]) * len(origins[1]) * len(origins[2]), bz, by, bx)


# ------------------------------------------------------------------------------------------------ steps 3 .. 6 per block
def block_correlate(volumes, template, G, taper, eps=1e-5, smooth=0.0):
    """The correlation maps fp32 [N, B, bz, by, bx]: section 30.1's steps 1 .. 4 on every block against its own template block."""
    bz, by, bx = G.block
    maps = []
    for oz in G.origins[0]:
        for oy in G.origins[1]:
            for ox in G.origins[2]:
                sl = (slice(oz, oz + bz), slice(oy, oy + by), slice(ox, ox + bx))
                maps.append(R3.correlate(volumes[(slice(None), *sl)], template[sl], taper, eps, smooth))
    return np.stack(maps, axis=1)


def block_shifts(volumes, template, G, max_shift, taper, smooth=0.0, eps=1e-5, subpixel=True):
    """(shifts fp32 [N, B, 3], peak fp32 [N, B])."""
    c = block_correlate(volumes, template, G, taper, eps, smooth)
    N, B = c.shape[:2]
    s, _, pk = R3.peak(c.reshape(N * B, *G.block), max_shift, subpixel)
    return s.reshape(N, B, 3), pk.reshape(N, B)


# ------------------------------------------------------------------------------------------------ step 7: the clean-up
def inliers(shifts, peak, base, min_peak=0.0, max_dev=None):
    """bool [N, B]; every comparison in float64 on the fp32 values."""
    s, pk, b = shifts.astype(F32).astype(np.float64), peak.astype(F32).astype(np.float64), base.astype(F32).astype(np.float64)
    with np.errstate(all="ignore"):
        ok = np.isfinite(pk) & (pk >= float(min_peak)) & np.isfinite(s).all(-1)
        if max_dev is not None:
            ok &= (np.abs(s - b[:, None, :]) <= np.asarray(max_dev, dtype=np.float64)).all(-1)
    return ok


def field_fill(shifts, peak, base, grid, min_peak=0.0, max_dev=None):
    """(field fp32 [N, B, 3], inlier uint8 [N, B])."""
    gz, gy, gx = grid
    N = shifts.shape[0]
    ok = inliers(shifts, peak, base, min_peak, max_dev)
    field = shifts.astype(F32).copy()
    for n in range(N):
        for iz in range(gz):
            for iy in range(gy):
                for ix in range(gx):
                    b = (iz * gy + iy) * gx + ix
                    if ok[n, b]:
                        continue
                    total, cnt = np.zeros(3, dtype=np.float64), 0
                    for dz in (-1, 0, 1):
                        for dy in (-1, 0, 1):
                            for dx in (-1, 0, 1):
                                z, y, x = iz + dz, iy + dy, ix + dx
                                if (dz, dy, dx) == (0, 0, 0) or not (0 <= z < gz and 0 <= y < gy and 0 <= x < gx):
                                    continue
                                nb = (z * gy + y) * gx + x
                                if ok[n, nb]:
                                    total = total + shifts[n, nb].astype(np.float64)
                                    cnt += 1
                    field[n, b] = (total / cnt).astype(F32) if cnt else base[n].astype(F32)
    return field, ok.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ step 8: the field and the warp
def lerp(a, b, t):
    """a where t == 0, else fl(a + fl(t * fl(b - a))), fp32 arrays."""
    a, b, t = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32), np.asarray(t, dtype=F32)
    with np.errstate(all="ignore"):
        r = (a + (t * (b - a).astype(F32)).astype(F32)).astype(F32)
    return np.where(t == 0, a, r).astype(F32)


def field_at(nodes, tabs):
    """fp32 [D, H, W, 3]: the node table [gz, gy, gx, 3] interpolated at every voxel: along x (four times), then y (twice), then z.
    Node i + 1 is clamped where t == 0 (lerp then returns a: the clamped value is not used)."""
    idxz, tz, idxy, ty, idxx, tx = tabs
    gz, gy, gx = nodes.shape[:3]
    z0, y0, x0 = idxz[:, None, None], idxy[None, :, None], idxx[None, None, :]
    z1, y1, x1 = np.minimum(z0 + 1, gz - 1), np.minimum(y0 + 1, gy - 1), np.minimum(x0 + 1, gx - 1)
    tz, ty, tx = tz[:, None, None, None], ty[None, :, None, None], tx[None, None, :, None]
    sh = (len(idxz), len(idxy), len(idxx), 3)
    at = lambda z, y, x: np.broadcast_to(nodes[z, y, x], sh)
    tx, ty, tz = np.broadcast_to(tx, sh), np.broadcast_to(ty, sh), np.broadcast_to(tz, sh)
    x00, x01 = lerp(at(z0, y0, x0), at(z0, y0, x1), tx), lerp(at(z0, y1, x0), at(z0, y1, x1), tx)
    x10, x11 = lerp(at(z1, y0, x0), at(z1, y0, x1), tx), lerp(at(z1, y1, x0), at(z1, y1, x1), tx)
    return lerp(lerp(x00, x01, ty), lerp(x10, x11, ty), tz)


def _gather(vol, zz, yy, xx, fill):
    D, H, W = vol.shape
    inside = (zz >= 0) & (zz < D) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    v = vol[np.clip(zz, 0, D - 1), np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(F32)
    return np.where(inside, v, F32(fill)).astype(F32)


def warp_volume(vol, d, mode="bilinear", fill=0.0):
    """One volume [D, H, W] under the displacement d [D, H, W, 3]: section 30.1's step 7 voxel by voxel -- the arithmetic of
    register_ref.shift in the plane (weights fl(wy_r * wx_c), taps (0,0), (0,1), (1,0), (1,1) added in that order, a zero weight
    skipped, nothing added: 0), the planes z + iz and the next blended as register3d_ref.shift blends them."""
    D, H, W = vol.shape
    Z, Y, X = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        d = d.astype(F32)
        bad = ~np.isfinite(d).all(-1)
        d = np.where(bad[..., None], F32(0), d)
        if mode == "nearest":
            d = np.rint(d).astype(F32)
        fl = np.floor(d).astype(F32)
        fr = (d - fl).astype(F32)
        lim = np.array([D + 1, H + 1, W + 1], dtype=F32)
        i = np.clip(fl, -lim, lim).astype(np.int64)
        w = [(F32(1) - fr[..., a], fr[..., a]) for a in range(3)]       # (w_0, w_1) per axis
        out, have_out = np.zeros((D, H, W), dtype=F32), np.zeros((D, H, W), dtype=bool)
        for rz in (0, 1):
            zz = Z + i[..., 0] + rz
            plane_in = (zz >= 0) & (zz < D)
            acc, have = np.zeros((D, H, W), dtype=F32), np.zeros((D, H, W), dtype=bool)
            for ry in (0, 1):
                for rx in (0, 1):
                    wt = (w[1][ry] * w[2][rx]).astype(F32)
                    use = wt != 0
                    tap = _gather(vol, zz, Y + i[..., 1] + ry, X + i[..., 2] + rx, fill)
                    term = (wt * np.where(use, tap, F32(0))).astype(F32)
                    acc = np.where(use, np.where(have, (acc + term).astype(F32), term), acc)
                    have |= use
            p = np.where(plane_in, acc, F32(fill)).astype(F32)          # nothing added inside the plane: acc is 0
            usez = w[0][rz] != 0
            term = (w[0][rz] * np.where(usez, p, F32(0))).astype(F32)
            out = np.where(usez, np.where(have_out, (out + term).astype(F32), term), out)
            have_out |= usez
        return np.where(bad, F32(fill), out).astype(F32)


def warp(x, field, G, mode="bilinear", fill=0.0):
    """fp32 [N, D, H, W]: every volume under its own interpolated field; ``field`` [N, B, 3] or [N, gz, gy, gx, 3]."""
    tabs = tables(G)
    return np.stack([warp_volume(v, field_at(np.asarray(f, dtype=F32).reshape(*G.grid, 3), tabs), mode, fill) for v, f in zip(x, field)])


# ------------------------------------------------------------------------------------------------ the planted scenes
Scene = namedtuple("Scene", ["volumes", "still", "table", "template", "grid"])


def canvas(seed, shape, pad, N=6, noise=0.02):
    """float64 [N, *(shape + 2 pad)]: the still scene of section 30.4 (register3d_ref.scene) on a padded canvas of any size, by the
    same recipe at the same density -- one Gaussian blob per 880 canvas voxels (sigma_z 0.8 - 1.4, sigma_xy 1 - 1.8, 300 - 900 counts),
    activity 0.35 + 0.65 [p < 0.6], bleaching exp(-0.02 n), background 120 +- 30, ``noise`` of the maximum on the canvas -- with every
    blob added on its own box of +-6 sigma, so that a canvas of 40 x 72 x 80 takes a fraction of a second."""
    rng = np.random.default_rng(5000 + seed)
    dims = np.array(shape) + 2 * np.array(pad)
    Dc, Hc, Wc = (int(v) for v in dims)
    n_blobs = max(8, int(round(Dc * Hc * Wc / 880.0)))
    cz, cy, cx = rng.uniform(1, Dc - 1, n_blobs), rng.uniform(2, Hc - 2, n_blobs), rng.uniform(2, Wc - 2, n_blobs)
    sz, sxy, amp = rng.uniform(0.8, 1.4, n_blobs), rng.uniform(1.0, 1.8, n_blobs), rng.uniform(300.0, 900.0, n_blobs)
    active = 0.35 + 0.65 * (rng.random((N, n_blobs)) < 0.6)
    zz, yy, xx = np.mgrid[0:Dc, 0:Hc, 0:Wc].astype(np.float64)
    cv = np.broadcast_to(120.0 + 30.0 * np.sin(yy / 9.0) * np.cos(xx / 11.0) * np.cos(zz / 5.0), (N, Dc, Hc, Wc)).copy()
    for k in range(n_blobs):
        lo = [max(0, int(np.floor(c - 6 * s))) for c, s in ((cz[k], sz[k]), (cy[k], sxy[k]), (cx[k], sxy[k]))]
        hi = [min(n, int(np.ceil(c + 6 * s)) + 1) for c, s, n in ((cz[k], sz[k], Dc), (cy[k], sxy[k], Hc), (cx[k], sxy[k], Wc))]
        z, y, x = np.mgrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].astype(np.float64)
        blob = np.exp(-(z - cz[k]) ** 2 / (2 * sz[k] ** 2) - ((y - cy[k]) ** 2 + (x - cx[k]) ** 2) / (2 * sxy[k] ** 2))
        cv[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += (active[:, k] * amp[k])[:, None, None, None] * blob[None]
    cv *= np.exp(-0.02 * np.arange(N))[:, None, None, None]
    return cv + noise * cv.max() * rng.standard_normal(cv.shape)


def _cells(G):
    """Per axis, the grid cell of every coordinate: the cells meet at the midpoints between neighbouring centres."""
    return [np.searchsorted((c[:-1] + c[1:]) / 2.0, np.arange(S, dtype=np.float64), side="right") for c, S in zip(G.centers, G.shape)]


def scene_p(seed, shape=(12, 48, 56), block=(12, 24, 28), grid=(1, 2, 2), N=6, max_d=(2, 3, 3), uniform=False):
    """(P) the piecewise-constant scene: every grid cell of volume n is the still canvas cut at its own integer displacement
    table[n, b] (volumes[n][p] = still[n][p - d]), |d| <= max_d; volume 0 does not move; ``uniform``: one d per volume."""
    G = block_grid(shape, block, grid)
    cv = canvas(seed, shape, max_d, N)
    rng = np.random.default_rng(7000 + seed)
    md = np.array(max_d)
    B = int(np.prod(G.grid))
    d = rng.integers(-md, md + 1, size=(N, 1 if uniform else B, 3))
    d = np.broadcast_to(d, (N, B, 3)).copy()
    d[0] = 0
    D, H, W = shape
    still = cv[:, md[0]:md[0] + D, md[1]:md[1] + H, md[2]:md[2] + W].astype(F32)
    cz, cy, cx = _cells(G)
    beta = (cz[:, None, None] * G.grid[1] + cy[None, :, None]) * G.grid[2] + cx[None, None, :]
    Z, Y, X = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    volumes = np.empty((N, D, H, W), dtype=F32)
    for n in range(N):
        dv = d[n][beta]                                                    # [D, H, W, 3]
        volumes[n] = cv[n][Z + md[0] - dv[..., 0], Y + md[1] - dv[..., 1], X + md[2] - dv[..., 2]].astype(F32)
    return Scene(volumes, still, d.astype(F32), R.lower_median(still), G)


def _sample(cv, q):
    """Trilinear sample of the float64 canvas at the float64 positions q [..., 3] (inside the canvas)."""
    i = np.floor(q).astype(np.int64)
    f = q - i
    out = np.zeros(q.shape[:-1], dtype=np.float64)
    for rz in (0, 1):
        for ry in (0, 1):
            for rx in (0, 1):
                wt = (f[..., 0] if rz else 1 - f[..., 0]) * (f[..., 1] if ry else 1 - f[..., 1]) * (f[..., 2] if rx else 1 - f[..., 2])
                out += wt * cv[np.clip(i[..., 0] + rz, 0, cv.shape[0] - 1), np.clip(i[..., 1] + ry, 0, cv.shape[1] - 1),
                               np.clip(i[..., 2] + rx, 0, cv.shape[2] - 1)]
    return out


def scene_s(seed, shape=(12, 48, 56), block=(12, 24, 28), grid=(1, 2, 2), N=6, max_d=(1.0, 2.0, 2.0)):
    """(S) the smooth scene: node vectors table[n, b] uniform in +-max_d (sub-voxel along z), volume 0 still; volume n is the canvas
    sampled in float64 at p - F_n(p), F_n the trilinear field of step 8 through those nodes."""
    G = block_grid(shape, block, grid)
    pad = tuple(int(np.ceil(m)) + 1 for m in max_d)
    cv = canvas(seed, shape, pad, N)
    rng = np.random.default_rng(9000 + seed)
    B = int(np.prod(G.grid))
    d = rng.uniform(-1.0, 1.0, size=(N, B, 3)) * np.array(max_d)
    d[0] = 0.0
    d = d.astype(F32)
    D, H, W = shape
    still = cv[:, pad[0]:pad[0] + D, pad[1]:pad[1] + H, pad[2]:pad[2] + W].astype(F32)
    P = np.stack(np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij"), axis=-1).astype(np.float64) + np.array(pad)
    volumes = np.stack([_sample(cv[n], P - field_at(d[n].reshape(*G.grid, 3), tables(G)).astype(np.float64)) for n in range(N)]).astype(F32)
    return Scene(volumes, still, d, R.lower_median(still), G)


def valid_mean_abs(a, b, box):
    z0, z1, y0, y1, x0, x1 = box
    return float(np.abs(a[:, z0:z1, y0:y1, x0:x1].astype(np.float64) - b[:, z0:z1, y0:y1, x0:x1].astype(np.float64)).mean())
