"""The numpy restatement of per-lenslet frame registration and the planted lenslet scene of its tests.

The label map, the cut-and-taper, the fit and the labelled resampling are spelled operation by operation; steps 2 to 7 of the
per-view estimate are ``register_ref``'s (and ``register_dft_ref``'s for ``subpixel="dft"``), called per view.  The fit is float64
with every sum taken over the views in order from 0.0 -- vectorised over the frames here, which does not change a frame's own
order of operations."""
from collections import namedtuple

import numpy as np

import register_ref as R

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ views and labels
def box_starts(centers, view_shape):
    c = np.asarray(centers, dtype=np.int64).reshape(-1, 2)
    return c[:, 0] - view_shape[0] // 2, c[:, 1] - view_shape[1] // 2


def label_map(shape, centers, view_shape):
    """uint8 [H, W]: the view whose box holds the pixel; the smallest integer squared distance to the centre among several, ties to
    the lowest index; L where none does."""
    H, W = shape
    ph, pw = view_shape
    c = np.asarray(centers, dtype=np.int64).reshape(-1, 2)
    L = len(c)
    y0, x0 = box_starts(c, view_shape)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    best = np.full((H, W), L, dtype=np.int64)
    bd = np.zeros((H, W), dtype=np.int64)
    for i in range(L):
        inside = (yy >= y0[i]) & (yy < y0[i] + ph) & (xx >= x0[i]) & (xx < x0[i] + pw)
        d = (yy - c[i, 0]) ** 2 + (xx - c[i, 1]) ** 2
        take = inside & ((best == L) | (d < bd))
        best[take], bd[take] = i, d[take]
    return best.astype(np.uint8)


def cut_views(x, centers, view_shape):
    """[N, L, ph, pw] of x's dtype: the boxes of every frame, pixels outside the frame 0."""
    N, H, W = x.shape
    ph, pw = view_shape
    y0, x0 = box_starts(centers, view_shape)
    out = np.zeros((N, len(y0), ph, pw), dtype=x.dtype)
    for i in range(len(y0)):
        ya, yb, xa, xb = max(0, y0[i]), min(H, y0[i] + ph), max(0, x0[i]), min(W, x0[i] + pw)
        if yb > ya and xb > xa:
            out[:, i, ya - y0[i]:yb - y0[i], xa - x0[i]:xb - x0[i]] = x[:, ya:yb, xa:xb]
    return out


def window_views(x, centers, view_shape, wy, wx):
    """fl(float(view) * fl(wy[y] * wx[x])), fp32 [N, L, ph, pw]."""
    return R.window(cut_views(x, centers, view_shape), wy, wx)


def estimate_view_shifts(frames, template, centers, view_shape, max_shift, taper, smooth=0.0, eps=1e-5, subpixel=True, u=16):
    """(shifts fp32 [N, L, 2], peak fp32 [N, L]): steps 1 to 6 of section 26.1 (26.5 for ``subpixel="dft"``) per view."""
    v, t = cut_views(frames, centers, view_shape), cut_views(template[None], centers, view_shape)[0]
    N, L = v.shape[:2]
    shifts, peak = np.zeros((N, L, 2), dtype=F32), np.zeros((N, L), dtype=F32)
    for i in range(L):
        if subpixel == "dft":
            import register_dft_ref as D
            shifts[:, i], peak[:, i] = D.estimate_shifts(v[:, i], t[i], max_shift, taper, smooth, eps, u=u)[:2]
        else:
            shifts[:, i], peak[:, i] = R.estimate_shifts(v[:, i], t[i], max_shift, taper, smooth, eps, subpixel)
    return shifts, peak


# ------------------------------------------------------------------------------------------------ the fit
def _fit_once(s, g, w):
    """(has a view, d_y, d_x, a) per frame from s float64 [N, L, 2], g float64 [L, 2] and the weights w bool [N, L]."""
    N, L = w.shape
    m, gy, gx, sy, sx = (np.zeros(N, dtype=F64) for _ in range(5))
    for i in range(L):
        wi = w[:, i]
        m = np.where(wi, m + 1.0, m)
        gy, gx = np.where(wi, gy + g[i, 0], gy), np.where(wi, gx + g[i, 1], gx)
        sy, sx = np.where(wi, sy + s[:, i, 0], sy), np.where(wi, sx + s[:, i, 1], sx)
    with np.errstate(all="ignore"):
        gy, gx, sy, sx = gy / m, gx / m, sy / m, sx / m
        q, c = np.zeros(N, dtype=F64), np.zeros(N, dtype=F64)
        for i in range(L):
            wi = w[:, i]
            ey, ex = g[i, 0] - gy, g[i, 1] - gx
            ty, tx = s[:, i, 0] - sy, s[:, i, 1] - sx
            q = np.where(wi, q + (ey * ey + ex * ex), q)
            c = np.where(wi, c + (ey * ty + ex * tx), c)
        a = np.where(q > 0.0, c / q, 0.0)
        dy, dx = sy - a * gy, sx - a * gx
    return m >= 1.0, dy, dx, a


Fit = namedtuple("Fit", ["table", "params", "inlier"])


def fit(shifts, peak, g, min_peak=0.0, reject=1.0, model="axial"):
    """``Fit(table fp32 [N, L+1, 2], params float64 [N, 3], inlier uint8 [N, L])``."""
    s, g = np.asarray(shifts, dtype=F32).astype(F64), np.asarray(g, dtype=F64)
    pk = np.asarray(peak, dtype=F32).astype(F64)
    N, L = pk.shape
    with np.errstate(all="ignore"):
        w = np.isfinite(pk) & (pk >= F64(min_peak))
        ok, dy, dx, a = _fit_once(s, g, w)
        ry = np.abs(s[:, :, 0] - (dy[:, None] + a[:, None] * g[None, :, 0]))
        rx = np.abs(s[:, :, 1] - (dx[:, None] + a[:, None] * g[None, :, 1]))
        gone = w & ok[:, None] & (np.where(ry > rx, ry, rx) > F64(reject))
        again = gone.any(1) & (w & ~gone).any(1)
        w = np.where(again[:, None], w & ~gone, w)                           # nothing left: the first fit and the first weights
        _, dy2, dx2, a2 = _fit_once(s, g, w)
        dy, dx, a = np.where(again, dy2, dy), np.where(again, dx2, dx), np.where(again, a2, a)
        dy, dx, a = np.where(ok, dy, 0.0), np.where(ok, dx, 0.0), np.where(ok, a, 0.0)
        table = np.empty((N, L + 1, 2), dtype=F32)
        table[:, :L, 0] = (dy[:, None] + a[:, None] * g[None, :, 0]).astype(F32)
        table[:, :L, 1] = (dx[:, None] + a[:, None] * g[None, :, 1]).astype(F32)
        table[:, L, 0], table[:, L, 1] = dy.astype(F32), dx.astype(F32)
    if model == "free":
        table[:, :L][w] = np.asarray(shifts, dtype=F32)[w]
    elif model != "axial":
        raise ValueError(model)
    return Fit(table, np.stack([dy, dx, a], axis=1), w.astype(np.uint8))


# ------------------------------------------------------------------------------------------------ the labelled resampling
def shift_labeled(x, table, labels, mode="bilinear", fill=0.0):
    """Step 7 of section 26.1 with (dy, dx) = table[n, min(labels[y, x], L)]: every label's pixels from ``register_ref.shift`` of the
    whole frame under that label's shift."""
    L = table.shape[1] - 1
    lab = np.minimum(labels.astype(np.int64), L)
    out = np.empty_like(x)
    for n in range(x.shape[0]):
        for l in np.unique(lab):
            m = lab == l
            out[n][m] = R.shift(x[n:n + 1], table[n, l][None], mode, fill)[0][m]
    return out


def valid_view_windows(table, centers, view_shape, shape):
    """int64 [L, 4] (y0, y1, x0, x1) in frame coordinates: where every frame's taps stay inside the view's box and the frame."""
    H, W = shape
    ph, pw = view_shape
    by, bx = box_starts(centers, view_shape)
    t = np.asarray(table, dtype=F64)
    out = np.zeros((len(by), 4), dtype=np.int64)
    for i in range(len(by)):
        lo, hi = np.array([max(by[i], 0), max(bx[i], 0)]), np.array([min(by[i] + ph, H), min(bx[i] + pw, W)])
        s = t[:, i]
        if s.size:
            if not np.isfinite(s).all():
                continue
            lo, hi = np.maximum(lo, lo - np.floor(s).min(0).astype(np.int64)), np.minimum(hi, hi - np.ceil(s).max(0).astype(np.int64))
        if (hi > lo).all():
            out[i] = lo[0], hi[0], lo[1], hi[1]
    return out


# ------------------------------------------------------------------------------------------------ the planted lenslet scene
LensletScene = namedtuple("LensletScene", ["frames", "still", "view_shifts", "d", "a", "template", "centers", "view_shape", "directions"])
VIEW = 48                                                                 # not below 48: DESIGN.md section 29.4
G = np.array([[0, 0], [0, 16], [0, -16], [16, 8], [16, -8], [-16, 8], [-16, -8]], dtype=F64)
CENTERS = (96 + 4 * G).astype(np.int32)                                   # a middle and six around it, 64 px apart along a row
FRAME = (192, 192)
DARK = 100.0


def _canvas(rng, Hc, Wc, N, n_blobs, noise):
    """The canvas of ``register_ref.scene``: blobs with intermittent activity and bleaching on a smooth background, plus noise."""
    yy, xx = np.mgrid[0:Hc, 0:Wc].astype(F64)
    cy, cx = rng.uniform(2, Hc - 2, n_blobs), rng.uniform(2, Wc - 2, n_blobs)
    sig, amp = rng.uniform(1.0, 1.8, n_blobs), rng.uniform(300.0, 900.0, n_blobs)
    blobs = np.stack([np.exp(-((yy - cy[k]) ** 2 + (xx - cx[k]) ** 2) / (2 * sig[k] ** 2)) for k in range(n_blobs)])
    active = 0.35 + 0.65 * (rng.random((N, n_blobs)) < 0.6)
    bleach = np.exp(-0.02 * np.arange(N))
    background = 120.0 + 30.0 * np.sin(yy / 9.0) * np.cos(xx / 11.0)
    canvas = bleach[:, None, None] * (background[None] + np.einsum("nk,kyx->nyx", active * amp[None, :], blobs))
    return canvas + noise * canvas.max() * rng.standard_normal(canvas.shape)


def lenslet_scene(seed, N=8, n_blobs=30, subpixel=False, noise=0.02):
    """N frames of FRAME with seven views of VIEW x VIEW, each an exact crop of its own canvas (8 px of padding) at the planted
    displacement d[n] + a[n] g_i (frames[p] = still[p - shift]); the pixels between the views are a dark level plus noise and do not
    move.  d in {-2 .. 2}^2 and a in {-1/8, 0, 1/8}: every per-view displacement is an integer of at most 4.  Frame 0 rests.
    ``subpixel``: d gets a fraction in (-0.5, 0.5) and every canvas is moved by a Fourier phase ramp before the cut."""
    rng = np.random.default_rng(2900 + seed)
    P, (H, W), L = R.PAD, FRAME, len(G)
    Hc = Wc = VIEW + 2 * P
    d = rng.integers(-2, 3, size=(N, 2)).astype(F64)
    a = rng.choice([-0.125, 0.0, 0.125], size=N)
    if N > 2:
        a[1], a[2] = 0.125, -0.125                                        # the fan opens and closes at least once
    if subpixel:
        d = d + rng.uniform(-0.5, 0.5, size=(N, 2))
    d[0], a[0] = 0.0, 0.0
    shifts = d[:, None, :] + a[:, None, None] * G[None]                   # [N, L, 2], exact in float64
    rest = DARK + noise * DARK * rng.standard_normal((N, H, W))
    frames, still = rest.astype(F32), rest.astype(F32)
    y0, x0 = box_starts(CENTERS, (VIEW, VIEW))
    ky, kx = np.fft.fftfreq(Hc)[:, None], np.fft.fftfreq(Wc)[None, :]
    for i in range(L):
        canvas = _canvas(rng, Hc, Wc, N, n_blobs, noise)
        still[:, y0[i]:y0[i] + VIEW, x0[i]:x0[i] + VIEW] = canvas[:, P:P + VIEW, P:P + VIEW].astype(F32)
        for n in range(N):
            iy, ix = int(np.floor(shifts[n, i, 0])), int(np.floor(shifts[n, i, 1]))
            fy, fx = shifts[n, i, 0] - iy, shifts[n, i, 1] - ix
            cv = canvas[n]
            if fy or fx:
                cv = np.fft.ifft2(np.fft.fft2(cv) * np.exp(-2j * np.pi * (ky * fy + kx * fx))).real
            frames[n, y0[i]:y0[i] + VIEW, x0[i]:x0[i] + VIEW] = cv[P - iy:P - iy + VIEW, P - ix:P - ix + VIEW].astype(F32)
    return LensletScene(frames, still, shifts.astype(F32), d, a, R.lower_median(still), CENTERS.copy(), (VIEW, VIEW), G.copy())


def second_peak_ratio(frames, template, centers, view_shape, taper, eps=1e-5):
    """The largest correlation value outside the 3 x 3 (cyclic) around the maximum, over the peak, worst over views and frames."""
    v, t = cut_views(frames, centers, view_shape), cut_views(template[None], centers, view_shape)[0]
    worst = 0.0
    for i in range(v.shape[1]):
        c = R.correlate(v[:, i], t[i], taper, eps)
        for n in range(c.shape[0]):
            y, x = np.unravel_index(np.argmax(c[n]), c[n].shape)
            rest = c[n].copy()
            rest[np.ix_([(y + k) % c.shape[1] for k in (-1, 0, 1)], [(x + k) % c.shape[2] for k in (-1, 0, 1)])] = -np.inf
            worst = max(worst, float(rest.max() / c[n, y, x]))
    return worst
