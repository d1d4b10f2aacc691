"""The numpy restatement of the up-sampled-DFT refinement of rigid frame registration.

It repeats the float64 operations of the three kernels of ``cwfa_reg_upsample_c64`` and of ``cwfa_reg_fine_peak_f64`` one at a time
and in their order: the root tables (octant reduction in integers, ``math.cos`` / ``math.sin``), the twiddles picked from them by an
index reduced in integers, the row sums over kx in order, the column sums over ky in eight segments, the uint64 order of the fine
maximum and the float64 parabola.  ``brute`` is the definition itself with ``numpy.exp``, for the rounding bounds of the CPU tests."""
import math

import numpy as np

import register_ref as R

F32, F64 = np.float32, np.float64
SEG = 8                                                                  # RUPS_SEG of register_ops.hip


# ------------------------------------------------------------------------------------------------ the tables and the twiddles
def reduce_octant(k, M):
    """2 pi k / M = pi p / q mirrored into [0, pi / 4]: (p, q, swap, sign of cos, sign of sin), all in integers."""
    p, q, sc, ss = 2 * k, M, 1.0, 1.0
    if p > q:
        p, ss = 2 * q - p, -1.0
    if 2 * p > q:
        p, sc = q - p, -1.0
    swap = 4 * p > q
    if swap:
        p, q = q - 2 * p, 2 * q
    return p, q, swap, sc, ss


def roots(M):
    """float64 [M, 2]: (cos, sin)(2 pi k / M), the angle formed as fl(fl(pi p) / q) after the reduction."""
    out = np.empty((M, 2), dtype=F64)
    for k in range(M):
        p, q, swap, sc, ss = reduce_octant(k, M)
        t = math.pi * p / q
        c, s = (math.sin(t), math.cos(t)) if swap else (math.cos(t), math.sin(t))
        out[k] = sc * c, ss * s
    return out


def twiddles(size, p, u, r, axis, root=None):
    """(re, im) float64 [k, U] of one frame: axis "x": w[kx] root[(kx m_j) mod (W u)], kx = 0 .. W/2; axis "y":
    root[(s(ky) m_j) mod (H u)], ky = 0 .. H - 1; m_j = (p u + j - r) mod (size u).  The Nyquist bin keeps its real part only."""
    M = size * u
    root = roots(M) if root is None else root
    m = [(int(p) * u + j) % M for j in range(-r, r + 1)]                   # Python's % is not negative
    if axis == "x":
        ks = list(range(size // 2 + 1))
        freq = ks
    else:
        ks = list(range(size))
        freq = [k if 2 * k < size else k - size for k in ks]
    idx = np.array([[(f * mj) % M for mj in m] for f in freq], dtype=np.int64)
    re, im = root[idx, 0].copy(), root[idx, 1].copy()
    if size % 2 == 0:
        im[size // 2] = 0.0
    if axis == "x":
        w = np.full(len(ks), 2.0)
        w[0] = 1.0
        if size % 2 == 0:
            w[size // 2] = 1.0
        re, im = w[:, None] * re, w[:, None] * im
    return re, im


# ------------------------------------------------------------------------------------------------ the two passes
def upsample(Rw, ipeak, shape, u, r=None, tables=None):
    """C float64 [N, U, U] from the spectra Rw complex64 [N, H, K] and the integer peaks [N, 2], operation by operation."""
    H, W = shape
    r = u if r is None else r
    N, K, U = Rw.shape[0], W // 2 + 1, 2 * r + 1
    assert Rw.shape[1:] == (H, K) and Rw.dtype == np.complex64
    rx, ry = tables if tables is not None else (roots(W * u), roots(H * u))
    inv = F64(1.0) / F64(H * W)
    L = (H + SEG - 1) // SEG
    C = np.empty((N, U, U), dtype=F64)
    with np.errstate(all="ignore"):
        for n in range(N):
            a, b = Rw[n].real.astype(F64), Rw[n].imag.astype(F64)         # [H, K]
            txr, txi = twiddles(W, ipeak[n][1], u, r, "x", rx)             # [K, U]
            tyr, tyi = twiddles(H, ipeak[n][0], u, r, "y", ry)             # [H, U]
            er, ei = np.zeros((H, U), dtype=F64), np.zeros((H, U), dtype=F64)
            for k in range(K):
                er = er + (a[:, k, None] * txr[None, k] - b[:, k, None] * txi[None, k])
                ei = ei + (a[:, k, None] * txi[None, k] + b[:, k, None] * txr[None, k])
            tot = np.zeros((U, U), dtype=F64)
            for s in range(SEG):
                part = np.zeros((U, U), dtype=F64)
                for y in range(min(s * L, H), min(s * L + L, H)):
                    part = part + (tyr[y][:, None] * er[y][None, :] - tyi[y][:, None] * ei[y][None, :])
                tot = tot + part
            C[n] = tot * inv
    return C


def brute(Rw, ipeak, shape, u, r=None):
    """The definition with numpy.exp in float64 / complex128, no stated order: what ``upsample`` is bounded against."""
    H, W = shape
    r = u if r is None else r
    N, K = Rw.shape[0], W // 2 + 1
    j = np.arange(-r, r + 1)
    w = np.full(K, 2.0)
    w[0] = 1.0
    if W % 2 == 0:
        w[W // 2] = 1.0
    sy = np.array([k if 2 * k < H else k - H for k in range(H)])
    out = np.empty((N, 2 * r + 1, 2 * r + 1))
    for n in range(N):
        py, px = int(ipeak[n][0]), int(ipeak[n][1])
        my, mx = (py * u + j) % (H * u), (px * u + j) % (W * u)
        tx = np.exp(2j * np.pi * ((np.arange(K)[:, None] * mx[None, :]) % (W * u)) / (W * u))
        ty = np.exp(2j * np.pi * ((sy[:, None] * my[None, :]) % (H * u)) / (H * u))
        if W % 2 == 0:
            tx[W // 2] = tx[W // 2].real
        if H % 2 == 0:
            ty[H // 2] = ty[H // 2].real
        out[n] = np.einsum("yj,yk,k,ki->ji", ty, Rw[n].astype(np.complex128), w, tx).real / (H * W)
    return out


# ------------------------------------------------------------------------------------------------ the fine peak
def ord64(v):
    """The order-preserving unsigned image of the float64 bits of v + 0.0; NaN -> 0."""
    v = np.asarray(v, dtype=F64) + F64(0)
    b = v.view(np.uint64)
    o = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(v), np.uint64(0), o).astype(np.uint64)


def delta64(a, b, c):
    """The parabola of register_ref.delta on float64 samples."""
    a, b, c = F64(a), F64(b), F64(c)
    with np.errstate(all="ignore"):
        den = (a - F64(2.0) * b) + c
        d = (F64(0.5) * (a - c)) / den
    if not (den < 0.0) or not np.isfinite(d):
        return 0.0
    return float(min(max(d, -0.5), 0.5))


def fine_peak(C, ipeak, u, shifts=None, peak=None):
    """(shifts fp32 [N,2], peak fp32 [N]).  ``shifts`` / ``peak`` given (the integer stage's): a frame whose peak is NaN is kept."""
    N, U = C.shape[0], C.shape[1]
    r = U // 2
    keep = peak is not None
    shifts = np.zeros((N, 2), dtype=F32) if shifts is None else np.array(shifts, dtype=F32)
    peak = np.zeros(N, dtype=F32) if peak is None else np.array(peak, dtype=F32)
    for n in range(N):
        if keep and np.isnan(peak[n]):
            continue
        py, px = int(ipeak[n][0]), int(ipeak[n][1])
        c = C[n].ravel()
        if not np.isfinite(c).any():
            shifts[n] = F32(float(py)), F32(float(px))
            peak[n] = np.nan
            continue
        o = ord64(c)
        i = int(np.flatnonzero(o == o.max())[0])                           # ties: the lowest row-major index
        jy, jx = divmod(i, U)
        dy = delta64(c[i - U], c[i], c[i + U]) if 0 < jy < U - 1 else 0.0
        dx = delta64(c[i - 1], c[i], c[i + 1]) if 0 < jx < U - 1 else 0.0
        shifts[n, 0] = F32(F64(py) + (F64(jy - r) + F64(dy)) / F64(u))
        shifts[n, 1] = F32(F64(px) + (F64(jx - r) + F64(dx)) / F64(u))
        with np.errstate(over="ignore"):
            peak[n] = F32(c[i])
    return shifts, peak


# ------------------------------------------------------------------------------------------------ end to end
def spectra(frames, template, taper, eps=1e-5, smooth=0.0):
    """The whitened cross-power complex64 [N, H, K] of register_ref.correlate (steps 1 to 3)."""
    N, H, W = frames.shape
    wy, wx = R.taper_window(H, taper), R.taper_window(W, taper)
    Wt = R.template_weight(template.astype(F32), wy, wx, eps, smooth)
    return np.stack([R.whiten(R.rfft2(R.window(frames[n], wy, wx)), Wt, eps) for n in range(N)])


def estimate_shifts(frames, template, max_shift, taper, smooth=0.0, eps=1e-5, u=16, tables=None):
    """``estimate_shifts(subpixel="dft", upsample=u)``: (shifts, peak, ipeak, C)."""
    N, H, W = frames.shape
    Rw = spectra(frames, template, taper, eps, smooth)
    corr = np.stack([R.irfft2(Rw[n], (H, W)) for n in range(N)])
    s, ip, pk = R.peak(corr, max_shift, subpixel=False)
    C = upsample(Rw, ip, (H, W), u, None, tables)
    s, pk = fine_peak(C, ip, u, s, pk)
    return s, pk, ip, C
