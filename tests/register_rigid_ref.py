"""The numpy restatement of the rigid registration of volumes with a rotation about the optical axis and the
planted scene of its tests.

The restatements of sections 30 and 32 (tests/register3d_ref.py, tests/register_blocks_ref.py) supply the table of block shifts, the
resampling of a voxel under its own vector and the rigid shift; this file adds the rigid fit of a table, its composition with a
prior motion, the displacement of a voxel under (dz, dy, dx, c, s) and the passes of the estimator, one rounding at a time."""
import math
from collections import namedtuple

import numpy as np

import register_ref as R
from register3d_ref import estimate_shifts, shift, valid_box
from register_blocks_ref import _sample, block_grid, block_shifts, canvas, valid_mean_abs, warp_volume

F32, F64 = np.float32, np.float64
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0)


# ------------------------------------------------------------------------------------------------ the geometry
def center(shape, c0=None):
    """(cy, cx) as two fp32 numbers: the given centre rounded once, or the centre of the plane."""
    if c0 is None:
        c0 = ((shape[-2] - 1) / 2.0, (shape[-1] - 1) / 2.0)
    return F32(c0[0]), F32(c0[1])


def arms(G, c0=None):
    """float64 [B, 2]: block centre minus rotation centre, (y, x), block b = (iz gy + iy) gx + ix."""
    cy, cx = center(G.shape, c0)
    gz, gy, gx = G.grid
    return np.array([[G.centers[1][iy] - F64(cy), G.centers[2][ix] - F64(cx)] for _ in range(gz) for iy in range(gy) for ix in range(gx)], dtype=F64)


def cm1_of(c, s):
    """c - 1 without cancellation: -(s s) / (1 + c), float64."""
    with np.errstate(all="ignore"):
        return F64(-(F64(s) * F64(s)) / (F64(1.0) + F64(c)))


# ------------------------------------------------------------------------------------------------ the fit
def _fit_once(s, a, w):
    """(dz, dy, dx, c, s) of one volume over the blocks of weight 1, or None where there is none; python floats are float64 and
    every operation below is rounded on its own."""
    B = len(w)
    m = ay = ax = sz = sy = sx = 0.0
    for b in range(B):
        if not w[b]:
            continue
        m = m + 1.0
        ay, ax = ay + a[b][0], ax + a[b][1]
        sz, sy, sx = sz + s[b][0], sy + s[b][1], sx + s[b][2]
    if not m >= 1.0:
        return None
    ay, ax, sz, sy, sx = ay / m, ax / m, sz / m, sy / m, sx / m
    P = Q = 0.0
    for b in range(B):
        if not w[b]:
            continue
        ey, ex = a[b][0] - ay, a[b][1] - ax
        fy, fx = ey + (s[b][1] - sy), ex + (s[b][2] - sx)
        P = P + (ey * fy + ex * fx)
        Q = Q + (ey * fx - ex * fy)
    with np.errstate(all="ignore"):
        r = float(np.sqrt(F64(P) * F64(P) + F64(Q) * F64(Q)))
        c, sn = 1.0, 0.0
        if r > 0.0 and P > 0.0:
            cc, ss = float(F64(P) / F64(r)), float(F64(Q) / F64(r))
            if math.isfinite(cc) and math.isfinite(ss):
                c, sn = cc, ss
    cm1 = float(cm1_of(c, sn))
    return sz, sy - (cm1 * ay - sn * ax), sx - (sn * ay + cm1 * ax), c, sn


def compose(prior, f):
    """The total motion prior o f of the original volume: R' R, R' d + d', dz + dz'."""
    dzp, dyp, dxp, cp, sp = (float(v) for v in prior)
    dz, dy, dx, c, s = f
    with np.errstate(all="ignore"):
        C, S = F64(cp * c - sp * s), F64(sp * c + cp * s)
        h = np.sqrt(C * C + S * S)
        cm1p = float(cm1_of(cp, sp))
        return (dz + dzp, (dy + (cm1p * dy - sp * dx)) + dyp, (dx + (sp * dy + cm1p * dx)) + dxp, float(C / h), float(S / h))


def fit(shifts, peak, a, min_peak=0.0, reject=1.0, prior=None, dtype=F32):
    """(params float64 [N, 5], inlier uint8 [N, B]) from shifts fp32 [N, B, 3], peak fp32 [N, B] and arms float64 [B, 2].  ``dtype``
    float64 keeps a float64 table as it is: the formulas alone, without the rounding of the measured shifts to fp32."""
    shifts, peak = np.asarray(shifts, dtype=dtype), np.asarray(peak, dtype=F32)
    N, B = peak.shape
    a = [[float(v) for v in row] for row in np.asarray(a, dtype=F64)]
    params, inlier = np.zeros((N, 5), dtype=F64), np.zeros((N, B), dtype=np.uint8)
    for n in range(N):
        s = [[float(v) for v in row] for row in shifts[n].astype(F64)]
        pk = [float(v) for v in peak[n].astype(F64)]
        w = [1 if math.isfinite(pk[b]) and pk[b] >= float(min_peak) and all(math.isfinite(v) for v in s[b]) else 0 for b in range(B)]
        f = _fit_once(s, a, w)
        if f is None:
            f = IDENTITY
        else:
            dz, dy, dx, c, sn = f
            cm1 = float(cm1_of(c, sn))
            w2 = list(w)
            for b in range(B):
                if not w[b]:
                    continue
                rz = abs(s[b][0] - dz)
                ry = abs(s[b][1] - (dy + (cm1 * a[b][0] - sn * a[b][1])))
                rx = abs(s[b][2] - (dx + (sn * a[b][0] + cm1 * a[b][1])))
                if max(rz, ry, rx) > float(reject):
                    w2[b] = 0
            if w2 != w and any(w2):
                w = w2
                f = _fit_once(s, a, w)
        params[n] = f if prior is None else compose(prior[n], f)
        inlier[n] = w
    return params, inlier


def table_of(params, a, dtype=F32):
    """[N, B, 3]: the block shifts the model predicts, u(p) = (dz, d + (R - I) a), formed in float64 and rounded once to ``dtype``."""
    out = np.zeros((len(params), len(a), 3), dtype=F64)
    for n, (dz, dy, dx, c, s) in enumerate(np.asarray(params, dtype=F64)):
        cm1 = cm1_of(c, s)
        out[n, :, 0] = dz
        out[n, :, 1] = dy + (cm1 * a[:, 0] - s * a[:, 1])
        out[n, :, 2] = dx + (s * a[:, 0] + cm1 * a[:, 1])
    return out.astype(dtype)


# ------------------------------------------------------------------------------------------------ the resampling
def displacement(p, shape, c0=None):
    """fp32 [H, W, 2] (vy, vx) and fp32 dz of one volume under p = (dz, dy, dx, c, s), or None where a parameter is not finite."""
    H, W = shape[-2:]
    cy, cx = center(shape, c0)
    dz, dy, dx, c, s = (F64(v) for v in p)
    with np.errstate(all="ignore"):
        dzf, dyf, dxf, sf, cm1f = F32(dz), F32(dy), F32(dx), F32(s), F32(cm1_of(c, s))
        if not (np.isfinite(c) and all(np.isfinite(v) for v in (dzf, dyf, dxf, sf, cm1f))):
            return None, None
        py = (np.arange(H, dtype=F32) - cy)[:, None]
        px = (np.arange(W, dtype=F32) - cx)[None, :]
        vy = dyf + ((cm1f * py).astype(F32) - (sf * px).astype(F32)).astype(F32)
        vx = dxf + ((sf * py).astype(F32) + (cm1f * px).astype(F32)).astype(F32)
    return dzf, np.stack((vy.astype(F32), vx.astype(F32)), axis=-1)


def move(x, params, c0=None, mode="bilinear", fill=0.0):
    """fp32 [N, D, H, W]: every volume resampled under its own (dz, dy, dx, c, s): the displacement of a voxel in fp32 as defined, then
    section 30.1's step 7 voxel by voxel (register_blocks_ref.warp_volume)."""
    x = np.asarray(x, dtype=F32)
    N, D, H, W = x.shape
    out = np.empty_like(x)
    for n in range(N):
        dzf, v = displacement(params[n], (D, H, W), c0)
        if v is None:
            out[n] = F32(fill)
            continue
        d = np.empty((D, H, W, 3), dtype=F32)
        d[..., 0], d[..., 1:] = dzf, v[None]
        out[n] = warp_volume(x[n], d, mode, fill)
    return out


def corner_shifts(params, shape, c0=None):
    """fp32 [4 N, 3]: (dz, vy, vx) at the four corners of the plane; NaN rows where a parameter is not finite."""
    rows = []
    for p in params:
        dzf, v = displacement(p, shape, c0)
        for y in (0, shape[1] - 1):
            for x in (0, shape[2] - 1):
                rows.append([np.nan] * 3 if v is None else [dzf, v[y, x, 0], v[y, x, 1]])
    return np.array(rows, dtype=F32).reshape(-1, 3)


def angles(params):
    return np.degrees(np.arctan2(params[:, 4], params[:, 3]))


# ------------------------------------------------------------------------------------------------ the estimator
def estimate(volumes, template, G, n_refine=2, c0=None, max_shift=(2, 8, 8), taper=(0, 0, 0), smooth=0.0, eps=1e-5, subpixel=True, min_peak=0.0,
             reject=1.0):
    """(params, peak, inlier, shifts, the params after every pass): pass 0 fits the table of the original volumes; every further
    pass moves the ORIGINAL volumes under the current motion, measures that table and fits with the current motion as prior."""
    a = arms(G, c0)
    shifts, peak = block_shifts(volumes, template, G, max_shift, taper, smooth, eps, subpixel)
    params, inlier = fit(shifts, peak, a, min_peak, reject)
    history = [params]
    for _ in range(n_refine):
        shifts, peak = block_shifts(move(volumes, params, c0), template, G, max_shift, taper, smooth, eps, subpixel)
        params, inlier = fit(shifts, peak, a, min_peak, reject, prior=params)
        history.append(params)
    return params, peak, inlier, shifts, history


def lever_bound(G, c0=None):
    """Radians: the angle error that half a voxel of error in every block shift can cause, 0.5 sum |e| / sum |e|^2, e = arm - mean arm
    (Q / P of the fit with every |f - R e| = 0.5 aligned with the tangent)."""
    e = arms(G, c0)
    e = e - e.mean(0)
    n = np.sqrt((e ** 2).sum(1))
    return 0.5 * n.sum() / (n ** 2).sum()


# ------------------------------------------------------------------------------------------------ the planted scene
Scene = namedtuple("Scene", ["volumes", "still", "params", "template", "grid"])
PAD = (1, 10, 10)


def scene(seed, shape=(8, 64, 72), block=(8, 32, 36), grid=(1, 3, 3), N=6, max_deg=3.0, max_d=2.0, c0=None):
    """N volumes of the canvas of section 32 (register_blocks_ref.canvas) sampled in float64 under a planted rotation about z, uniform
    in +-max_deg, and a planted sub-voxel in-plane shift, uniform in +-max_d per axis; volume 0 does not move.  With the planted
    params (0, dy, dx, cos, sin), volumes[n](q) = still[n](c0 + R^T (q - c0 - d)): ``move`` under them gives back the still scene."""
    G = block_grid(shape, block, grid)
    cv = canvas(seed, shape, PAD, N)
    rng = np.random.default_rng(11000 + seed)
    theta = np.radians(rng.uniform(-max_deg, max_deg, N))
    d = rng.uniform(-max_d, max_d, (N, 2))
    theta[0], d[0] = 0.0, 0.0
    D, H, W = shape
    cy, cx = (F64(v) for v in center(shape, c0))
    still = cv[:, PAD[0]:PAD[0] + D, PAD[1]:PAD[1] + H, PAD[2]:PAD[2] + W].astype(F32)
    Z, Y, X = (g.astype(F64) for g in np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij"))
    volumes = np.empty((N, D, H, W), dtype=F32)
    for n in range(N):
        c, s = np.cos(theta[n]), np.sin(theta[n])
        qy, qx = Y - cy - d[n, 0], X - cx - d[n, 1]
        q = np.stack((Z + PAD[0], cy + (c * qy + s * qx) + PAD[1], cx + (-s * qy + c * qx) + PAD[2]), axis=-1)
        volumes[n] = _sample(cv[n], q).astype(F32)
    params = np.stack((np.zeros(N), d[:, 0], d[:, 1], np.cos(theta), np.sin(theta)), axis=1)
    return Scene(volumes, still, params, R.lower_median(still), G)


def both_boxes(params, shifts, shape, c0=None):
    """The box that holds data after the rigid motion ``params`` AND after the plain shifts ``shifts``."""
    a, b = valid_box(corner_shifts(params, shape, c0), shape), valid_box(shifts, shape)
    box = tuple(max(a[k], b[k]) if k % 2 == 0 else min(a[k], b[k]) for k in range(6))
    return box if all(box[k + 1] > box[k] for k in (0, 2, 4)) else (0,) * 6


def translation_only(volumes, template, max_shift, taper):
    """(registered volumes, shifts) of section 30: one vector per volume."""
    s, _ = estimate_shifts(volumes, template, max_shift, taper)
    return shift(volumes, s), s


__all__ = ["center", "arms", "cm1_of", "fit", "compose", "table_of", "displacement", "move", "corner_shifts", "angles", "estimate", "lever_bound",
           "scene", "Scene", "both_boxes", "translation_only", "valid_mean_abs", "valid_box", "shift", "block_shifts", "canvas"]
