"""The numpy restatement of the rigid registration of volumes and the planted scene of its tests.

The 2-D restatement (tests/register_ref.py) supplies the taper, the whitening, the key order, the parabola and the in-plane
resampling; this file adds the third axis, one rounding at a time.  The transforms are ``numpy.fft`` in float64, rounded to
complex64 / float32 -- the one place where the device (rocFFT, fp32) and this file differ, which is why the kernels are tested on
handed-in maps."""
from collections import namedtuple

import numpy as np

import register_ref as R

F32 = np.float32


# ------------------------------------------------------------------------------------------------ steps 1 .. 4
def window(x, wz, wy, wx):
    """fl(x * fl(fl(wz[z] * wy[y]) * wx[x])), fp32 [.., D, H, W]."""
    w2 = wz.astype(F32)[:, None] * wy.astype(F32)[None, :]                 # rounded to fp32
    w3 = w2[:, :, None] * wx.astype(F32)[None, None, :]
    return x.astype(F32) * w3


def rfftn(x):
    return np.fft.rfftn(x.astype(np.float64), axes=(-3, -2, -1)).astype(np.complex64)


def irfftn(Rs, shape):
    return np.fft.irfftn(Rs.astype(np.complex128), s=shape, axes=(-3, -2, -1)).astype(F32)


def lowpass(D, H, W, smooth):
    kz, ky, kx = np.fft.fftfreq(D), np.fft.fftfreq(H), np.fft.rfftfreq(W)
    k2 = kz[:, None, None] ** 2 + ky[None, :, None] ** 2 + kx[None, None, :] ** 2
    return np.exp(-2.0 * np.pi ** 2 * float(smooth) ** 2 * k2).astype(F32)


def tapers(shape, taper):
    t = (taper,) * 3 if isinstance(taper, int) else tuple(taper)
    return tuple(R.taper_window(n, k) for n, k in zip(shape, t))


def template_weight(template, wins, eps=1e-5, smooth=0.0):
    U = R.whiten(rfftn(window(template, *wins)), None, eps)
    ur, ui = U.real.astype(F32), U.imag.astype(F32)
    Wt = np.empty(U.shape, dtype=np.complex64)
    if smooth > 0.0:
        G = lowpass(*template.shape, smooth)
        Wt.real, Wt.imag = ur * G, -ui * G
    else:
        Wt.real, Wt.imag = ur, -ui
    Wt[0, 0, 0] = 0
    return Wt


def correlate(volumes, template, taper, eps=1e-5, smooth=0.0):
    """Steps 1 to 4: the correlation maps fp32 [N, D, H, W]."""
    shape = volumes.shape[1:]
    wins = tapers(shape, taper)
    Wt = template_weight(template.astype(F32), wins, eps, smooth)
    return np.stack([irfftn(R.whiten(rfftn(window(v, *wins)), Wt, eps), shape) for v in volumes])


# ------------------------------------------------------------------------------------------------ steps 5 and 6
def _m3(max_shift):
    return (max_shift,) * 3 if isinstance(max_shift, (int, np.integer)) else tuple(int(m) for m in max_shift)


def window_keys(c, mz, my, mx):
    """uint64 keys of the search window of one map, row-major from (-mz, -my, -mx), and the window's values."""
    D, H, W = c.shape
    sz, sy, sx = np.arange(-mz, mz + 1), np.arange(-my, my + 1), np.arange(-mx, mx + 1)
    vals = c[np.mod(sz, D)[:, None, None], np.mod(sy, H)[None, :, None], np.mod(sx, W)[None, None, :]].ravel()
    idx = np.arange(vals.size, dtype=np.uint64)
    return (R.ord32(vals).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx), vals


def peak(c, max_shift, subpixel=True):
    """(shifts fp32 [N,3], ipeak int32 [N,3], peak fp32 [N]) of the maps c [N,D,H,W]."""
    mz, my, mx = _m3(max_shift)
    N, D, H, W = c.shape
    assert 2 * mz + 1 <= D and 2 * my + 1 <= H and 2 * mx + 1 <= W
    shifts, ip, pk = np.zeros((N, 3), dtype=F32), np.zeros((N, 3), dtype=np.int32), np.zeros(N, dtype=F32)
    wh, ww = 2 * my + 1, 2 * mx + 1
    for n in range(N):
        keys, vals = window_keys(c[n], mz, my, mx)
        if not np.isfinite(vals).any():
            pk[n] = np.nan
            continue
        i = int(np.uint64(0xFFFFFFFF) - (keys.max() & np.uint64(0xFFFFFFFF)))
        sz, sy, sx = i // (wh * ww) - mz, (i // ww) % wh - my, i % ww - mx
        z, y, x = sz % D, sy % H, sx % W
        dz = dy = dx = 0.0
        if subpixel:
            dz = R.delta(c[n, (z - 1) % D, y, x], c[n, z, y, x], c[n, (z + 1) % D, y, x])
            dy = R.delta(c[n, z, (y - 1) % H, x], c[n, z, y, x], c[n, z, (y + 1) % H, x])
            dx = R.delta(c[n, z, y, (x - 1) % W], c[n, z, y, x], c[n, z, y, (x + 1) % W])
        shifts[n] = F32(float(sz) + dz), F32(float(sy) + dy), F32(float(sx) + dx)
        ip[n] = sz, sy, sx
        pk[n] = c[n, z, y, x]
    return shifts, ip, pk


# ------------------------------------------------------------------------------------------------ step 7
def shift(x, shifts, mode="bilinear", fill=0.0):
    """out[n,z] = fl(wz0 * p_0) + fl(wz1 * p_1), p_r = the 2-D restatement's resampling of plane z + iz + r under (dy, dx), a plane
    outside the volume holding ``fill``; a plane of weight 0 is skipped."""
    N, D, H, W = x.shape
    out = np.empty_like(x)
    for n in range(N):
        dz, dy, dx = (F32(v) for v in shifts[n])
        if not (np.isfinite(dz) and np.isfinite(dy) and np.isfinite(dx)):
            out[n] = F32(fill)
            continue
        if mode == "nearest":
            dz = np.rint(dz)                                               # the 2-D restatement rounds (dy, dx) itself
        izf = np.floor(dz)
        fz = F32(dz - izf)
        iz = int(np.clip(izf, -(D + 1), D + 1))
        wz = (F32(F32(1) - fz), fz)
        planes = R.shift(x[n], np.tile(np.array([[dy, dx]], dtype=F32), (D, 1)), mode, fill)      # every plane under (dy, dx)
        with np.errstate(all="ignore"):
            for z in range(D):
                acc = None
                for r in (0, 1):
                    if wz[r] == 0:
                        continue
                    zz = z + iz + r
                    p = planes[zz] if 0 <= zz < D else np.full((H, W), F32(fill), dtype=F32)
                    t = wz[r] * p
                    acc = t if acc is None else acc + t
                out[n, z] = acc
    return out


def estimate_shifts(volumes, template, max_shift, taper, smooth=0.0, eps=1e-5, subpixel=True):
    s, _, pk = peak(correlate(volumes, template, taper, eps, smooth), max_shift, subpixel)
    return s, pk


def valid_box(shifts, shape):
    s = np.asarray(shifts, dtype=np.float64).reshape(-1, 3)
    if s.size == 0:
        return 0, shape[0], 0, shape[1], 0, shape[2]
    if not np.isfinite(s).all():
        return (0,) * 6
    lo, hi = np.floor(s).min(0), np.ceil(s).max(0)
    box = []
    for a in range(3):
        b0, b1 = max(0, int(-lo[a])), min(shape[a], shape[a] - int(hi[a]))
        if b1 <= b0:
            return (0,) * 6
        box += [b0, b1]
    return tuple(box)


# ------------------------------------------------------------------------------------------------ the planted scene
Scene = namedtuple("Scene", ["volumes", "still", "shifts", "template"])
PAD = (4, 8, 8)


def scene(seed, D=12, H=24, W=28, N=6, n_blobs=40, max_d=(2, 3, 3), subpixel=False, noise=0.02, rest=0):
    """N volumes of Gaussian blobs (sigma_z 0.8 - 1.4, sigma_xy 1 - 1.8 voxels, 300 - 900 counts) with intermittent activity (a floor
    of 0.35 plus 0.65 with probability 0.6) and bleaching exp(-0.02 n) on a smooth background of 120 +- 30, 2 % noise already on the
    still canvas, which is padded by PAD; volume n is the canvas cut at the planted displacement d[n]
    (volumes[n][p] = still[n][p - d[n]]; volume 0 does not move).  Integer d: an exact crop.  ``subpixel``: d has a fractional part
    and the canvas is moved by a 3-D Fourier phase ramp before the cut.  ``rest``: that many further volumes do not move either.
    ``template``: the lower median of the still volumes."""
    rng = np.random.default_rng(3000 + seed)
    shape = np.array([D, H, W])
    pad = np.array(PAD)
    Dc, Hc, Wc = shape + 2 * pad
    zz, yy, xx = np.mgrid[0:Dc, 0:Hc, 0:Wc].astype(np.float64)
    cz, cy, cx = rng.uniform(1, Dc - 1, n_blobs), rng.uniform(2, Hc - 2, n_blobs), rng.uniform(2, Wc - 2, n_blobs)
    sz, sxy, amp = rng.uniform(0.8, 1.4, n_blobs), rng.uniform(1.0, 1.8, n_blobs), rng.uniform(300.0, 900.0, n_blobs)
    blobs = np.stack([np.exp(-(zz - cz[k]) ** 2 / (2 * sz[k] ** 2) - ((yy - cy[k]) ** 2 + (xx - cx[k]) ** 2) / (2 * sxy[k] ** 2))
                      for k in range(n_blobs)])
    active = 0.35 + 0.65 * (rng.random((N, n_blobs)) < 0.6)
    bleach = np.exp(-0.02 * np.arange(N))
    background = 120.0 + 30.0 * np.sin(yy / 9.0) * np.cos(xx / 11.0) * np.cos(zz / 5.0)
    canvas = bleach[:, None, None, None] * (background[None] + np.einsum("nk,kzyx->nzyx", active * amp[None, :], blobs))
    canvas = canvas + noise * canvas.max() * rng.standard_normal(canvas.shape)
    md = np.array(max_d)
    d = rng.integers(-md, md + 1, size=(N, 3)).astype(np.float64)
    if subpixel:
        d = np.clip(d + rng.uniform(-0.5, 0.5, size=(N, 3)), -md, md)
    d[:1 + rest] = 0.0
    still = canvas[:, pad[0]:pad[0] + D, pad[1]:pad[1] + H, pad[2]:pad[2] + W].astype(F32)
    volumes = np.empty((N, D, H, W), dtype=F32)
    kz, ky, kx = np.fft.fftfreq(Dc)[:, None, None], np.fft.fftfreq(Hc)[None, :, None], np.fft.fftfreq(Wc)[None, None, :]
    for n in range(N):
        i = np.floor(d[n]).astype(int)
        f = d[n] - i
        cv = canvas[n]
        if f.any():                                                        # the canvas moved by the fraction, band-limited
            cv = np.fft.ifftn(np.fft.fftn(cv) * np.exp(-2j * np.pi * (kz * f[0] + ky * f[1] + kx * f[2]))).real
        o = pad - i
        volumes[n] = cv[o[0]:o[0] + D, o[1]:o[1] + H, o[2]:o[2] + W].astype(F32)
    return Scene(volumes, still, d.astype(F32), R.lower_median(still))
