"""The numpy restatement of rigid frame registration and the planted scene of its tests.

The restatement spells every rounding of the four HIP passes: fp32 products and sums one at a time, uint64 keys for the peak,
float64 for the parabola.  The transforms are ``numpy.fft`` in float64, rounded to complex64 / float32 -- the one place where the
device (rocFFT, fp32) and this file differ, which is why the kernels are tested on handed-in spectra and maps."""
from collections import namedtuple

import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------ steps 1 .. 4
def taper_window(n, taper):
    """0.5 - 0.5 cos(pi (i + 0.5) / taper) on both ends, 1 inside; float64 rounded once to fp32."""
    w = np.ones(n, dtype=np.float64)
    if taper:
        edge = 0.5 - 0.5 * np.cos(np.pi * (np.arange(taper, dtype=np.float64) + 0.5) / taper)
        w[:taper] = edge
        w[n - taper:] = edge[::-1]
    return w.astype(F32)


def window(x, wy, wx):
    """fl(float(x) * fl(wy[y] * wx[x])), fp32 [.., H, W]."""
    w2 = wy.astype(F32)[:, None] * wx.astype(F32)[None, :]
    return x.astype(F32) * w2


def rfft2(x):
    return np.fft.rfft2(x.astype(np.float64)).astype(np.complex64)


def irfft2(R, shape):
    return np.fft.irfft2(R.astype(np.complex128), s=shape).astype(F32)


def whiten(F, W=None, eps=1e-5):
    """z / (|z| + eps) with |z| = sqrtf(fl(fl(re re) + fl(im im))), times W where given: each operation rounded to fp32."""
    re, im = np.ascontiguousarray(F.real, dtype=F32), np.ascontiguousarray(F.imag, dtype=F32)
    with np.errstate(all="ignore"):
        m = np.sqrt(re * re + im * im)
        d = m + F32(eps)
        ur, ui = re / d, im / d
        if W is not None:
            wr, wi = np.ascontiguousarray(W.real, dtype=F32), np.ascontiguousarray(W.imag, dtype=F32)
            ur, ui = ur * wr - ui * wi, ur * wi + ui * wr
    out = np.empty(F.shape, dtype=np.complex64)
    out.real, out.imag = ur, ui
    return out


def lowpass(H, W, smooth):
    ky, kx = np.fft.fftfreq(H), np.fft.rfftfreq(W)
    return np.exp(-2.0 * np.pi ** 2 * float(smooth) ** 2 * (ky[:, None] ** 2 + kx[None, :] ** 2)).astype(F32)


def template_weight(template, wy, wx, eps=1e-5, smooth=0.0):
    H, W = template.shape
    U = whiten(rfft2(window(template, wy, wx)), None, eps)
    ur, ui = U.real.astype(F32), U.imag.astype(F32)
    Wt = np.empty(U.shape, dtype=np.complex64)
    if smooth > 0.0:
        G = lowpass(H, W, smooth)
        Wt.real, Wt.imag = ur * G, -ui * G
    else:
        Wt.real, Wt.imag = ur, -ui
    Wt[0, 0] = 0
    return Wt


def correlate(frames, template, taper, eps=1e-5, smooth=0.0):
    """Steps 1 to 4: the correlation maps fp32 [N, H, W]."""
    N, H, W = frames.shape
    wy, wx = taper_window(H, taper), taper_window(W, taper)
    Wt = template_weight(template.astype(F32), wy, wx, eps, smooth)
    return np.stack([irfft2(whiten(rfft2(window(frames[n], wy, wx)), Wt, eps), (H, W)) for n in range(N)])


# ------------------------------------------------------------------------------------------------ steps 5 and 6
def ord32(v):
    """The order-preserving unsigned image of the fp32 bits of v + 0.0f; NaN -> 0."""
    v = np.asarray(v, dtype=F32) + F32(0)
    u = v.view(np.uint32)
    o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(v), np.uint32(0), o)


def window_keys(c, my, mx):
    """uint64 keys of the search window of one map, row-major from (-my, -mx), and the window's values."""
    H, W = c.shape
    sy, sx = np.arange(-my, my + 1), np.arange(-mx, mx + 1)
    vals = c[np.mod(sy, H)[:, None], np.mod(sx, W)[None, :]].ravel()
    idx = np.arange(vals.size, dtype=np.uint64)
    return (ord32(vals).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx), vals


def delta(cm, c0, cp):
    """The parabola's vertex from three fp32 samples, in float64."""
    a, b, c = float(F32(cm)), float(F32(c0)), float(F32(cp))
    with np.errstate(all="ignore"):
        den = np.float64(a) - np.float64(2.0) * np.float64(b) + np.float64(c)
        d = (np.float64(0.5) * (np.float64(a) - np.float64(c))) / den
    if not (den < 0.0) or not np.isfinite(d):
        return 0.0
    return float(min(max(d, -0.5), 0.5))


def peak(c, max_shift, subpixel=True):
    """(shifts fp32 [N,2], ipeak int32 [N,2], peak fp32 [N]) of the maps c [N,H,W]."""
    my, mx = (max_shift, max_shift) if isinstance(max_shift, int) else max_shift
    N, H, W = c.shape
    assert 2 * my + 1 <= H and 2 * mx + 1 <= W
    shifts, ip, pk = np.zeros((N, 2), dtype=F32), np.zeros((N, 2), dtype=np.int32), np.zeros(N, dtype=F32)
    ww = 2 * mx + 1
    for n in range(N):
        keys, vals = window_keys(c[n], my, mx)
        if not np.isfinite(vals).any():
            pk[n] = np.nan
            continue
        i = int(np.uint64(0xFFFFFFFF) - (keys.max() & np.uint64(0xFFFFFFFF)))
        sy, sx = i // ww - my, i % ww - mx
        y, x = sy % H, sx % W
        dy = delta(c[n, (y - 1) % H, x], c[n, y, x], c[n, (y + 1) % H, x]) if subpixel else 0.0
        dx = delta(c[n, y, (x - 1) % W], c[n, y, x], c[n, y, (x + 1) % W]) if subpixel else 0.0
        shifts[n] = F32(float(sy) + dy), F32(float(sx) + dx)
        ip[n] = sy, sx
        pk[n] = c[n, y, x]
    return shifts, ip, pk


# ------------------------------------------------------------------------------------------------ step 7
def _tap(src, oy, ox, fill):
    """src[y + oy, x + ox] as fp32, ``fill`` outside."""
    H, W = src.shape
    out = np.full((H, W), F32(fill), dtype=F32)
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = src[y0 + oy:y1 + oy, x0 + ox:x1 + ox].astype(F32)
    return out


def shift(x, shifts, mode="bilinear", fill=0.0):
    """out[n,y,x] = sum of w * x[n, y + iy + r, x + ix + c] over the taps (0,0), (0,1), (1,0), (1,1); a zero weight is skipped."""
    N, H, W = x.shape
    out = np.empty_like(x)
    for n in range(N):
        dy, dx = F32(shifts[n, 0]), F32(shifts[n, 1])
        if not (np.isfinite(dy) and np.isfinite(dx)):
            out[n] = F32(fill)
            continue
        if mode == "nearest":
            dy, dx = np.rint(dy), np.rint(dx)
        iyf, ixf = np.floor(dy), np.floor(dx)
        fy, fx = F32(dy - iyf), F32(dx - ixf)
        iy, ix = int(np.clip(iyf, -(H + 1), H + 1)), int(np.clip(ixf, -(W + 1), W + 1))
        wyv, wxv = (F32(1) - fy, fy), (F32(1) - fx, fx)
        acc = None
        with np.errstate(all="ignore"):
            for r in (0, 1):
                for c in (0, 1):
                    w = F32(wyv[r] * wxv[c])
                    if w == 0:
                        continue
                    t = w * _tap(x[n], iy + r, ix + c, fill)
                    acc = t if acc is None else acc + t
            out[n] = (np.zeros((H, W), dtype=F32) if acc is None else acc).astype(x.dtype)
    return out


def estimate_shifts(frames, template, max_shift, taper, smooth=0.0, eps=1e-5, subpixel=True):
    s, _, pk = peak(correlate(frames, template, taper, eps, smooth), max_shift, subpixel)
    return s, pk


def lower_median(x):
    """The per-pixel temporal median by the rank rule of numpy.quantile(method="lower")."""
    return np.sort(x, axis=0)[(x.shape[0] - 1) // 2]


def valid_window(shifts, shape):
    H, W = shape
    s = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    lo, hi = np.floor(s).min(0), np.ceil(s).max(0)
    return max(0, int(-lo[0])), min(H, H - int(hi[0])), max(0, int(-lo[1])), min(W, W - int(hi[1]))


# ------------------------------------------------------------------------------------------------ the planted scene
Scene = namedtuple("Scene", ["frames", "still", "shifts", "template"])
PAD = 8


def scene(seed, H=37, W=45, N=8, n_blobs=30, max_d=4, subpixel=False, noise=0.02, rest=0):
    """N frames of Gaussian blobs (sigma 1 - 1.8 px) with intermittent activity and slow bleaching on a smooth background, noise
    already on the still canvas [N, H + 2 PAD, W + 2 PAD]; frame n is the canvas cut at the planted displacement d[n]
    (frames[n][p] = still[n][p - d[n]]; frame 0 does not move).  Integer d: an exact crop.  ``subpixel``: d has a fractional part
    and the canvas is moved by a Fourier phase ramp before the cut.  ``rest``: that many further frames do not move either (a
    sample that rests and twitches: the moved stack's own median is then a usable template).  ``template``: the lower median of
    the still frames."""
    rng = np.random.default_rng(1000 + seed)
    Hc, Wc = H + 2 * PAD, W + 2 * PAD
    yy, xx = np.mgrid[0:Hc, 0:Wc].astype(np.float64)
    cy, cx = rng.uniform(2, Hc - 2, n_blobs), rng.uniform(2, Wc - 2, n_blobs)
    sig, amp = rng.uniform(1.0, 1.8, n_blobs), rng.uniform(300.0, 900.0, n_blobs)
    blobs = np.stack([np.exp(-((yy - cy[k]) ** 2 + (xx - cx[k]) ** 2) / (2 * sig[k] ** 2)) for k in range(n_blobs)])
    active = 0.35 + 0.65 * (rng.random((N, n_blobs)) < 0.6)              # a floor of resting fluorescence, transients on top
    bleach = np.exp(-0.02 * np.arange(N))
    background = 120.0 + 30.0 * np.sin(yy / 9.0) * np.cos(xx / 11.0)
    canvas = bleach[:, None, None] * (background[None] + np.einsum("nk,kyx->nyx", active * amp[None, :], blobs))
    canvas = canvas + noise * canvas.max() * rng.standard_normal(canvas.shape)
    d = rng.integers(-max_d, max_d + 1, size=(N, 2)).astype(np.float64)
    if subpixel:
        d = d + rng.uniform(-0.5, 0.5, size=(N, 2))
        d = np.clip(d, -max_d, max_d)
    d[:1 + rest] = 0.0
    still = canvas[:, PAD:PAD + H, PAD:PAD + W].astype(F32)
    frames = np.empty((N, H, W), dtype=F32)
    ky, kx = np.fft.fftfreq(Hc)[:, None], np.fft.fftfreq(Wc)[None, :]
    for n in range(N):
        iy, ix = int(np.floor(d[n, 0])), int(np.floor(d[n, 1]))
        fy, fx = d[n, 0] - iy, d[n, 1] - ix
        cv = canvas[n]
        if fy or fx:                                                   # the canvas moved by the fraction, band-limited
            cv = np.fft.ifft2(np.fft.fft2(cv) * np.exp(-2j * np.pi * (ky * fy + kx * fx))).real
        frames[n] = cv[PAD - iy:PAD - iy + H, PAD - ix:PAD - ix + W].astype(F32)
    return Scene(frames, still, d.astype(F32), lower_median(still))
