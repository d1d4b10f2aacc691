"""Restatement of cwfa_rand_poisson_f32 in numpy, every decision in ``dtype`` (float64: what the kernel
evaluates; numpy.longdouble: the check that float64 decides every draw the way a wider format does).  Philox from sampler_ref.

Counters (NOT those of cwfa_rand_uniform_f32, which packs four elements into a block): element e of sample s, round t, uses the
block with counter (e & 0xffffffff, (e >> 32) | (t << 20), sample_offset + s, stream) under the key (seed & 0xffffffff, seed >> 32);
a word r becomes u = (r + 0.5) 2^-32.  rate = fl32(lam * pre) in float32, then:
  rate < 10    inversion by sequential search on word 0 of round 0, at most 80 steps;
  rate >= 10   Hoermann's PTRS; attempt j takes (U, V) from words (2 (j & 1), 2 (j & 1) + 1) of round j >> 1, at most 64 attempts,
               then k = rint(rate);
  rate = 0 -> 0;  rate negative, NaN or above 2^30 -> NaN.
out = fl32(fl32(k) * post)."""
import math

import numpy as np

import sampler_ref as S

try:
    from scipy.special import gammaln as _gammaln
except ImportError:                                                        # pragma: no cover
    _gammaln = np.vectorize(math.lgamma, otypes=[np.float64])

MASK = S.MASK
SMALL, RATE_MAX, MAX_STEPS, MAX_ROUNDS = 10.0, 2.0 ** 30, 80, 32


def lgamma(x, dtype):
    """log Gamma(x), x >= 1.  float64: scipy's (or math.lgamma).  longdouble: Stirling's series after shifting x to >= 32 with the
    recurrence (truncation below 1e-22 relative), so that it owes nothing to the float64 routine it is compared with."""
    if dtype is np.float64:
        return _gammaln(x)
    x = np.asarray(x, dtype=dtype)
    shift = np.zeros_like(x)
    y = x.copy()
    for _ in range(32):                                                    # log Gamma(x) = log Gamma(x + m) - log(x (x+1) .. (x+m-1))
        low = y < 32
        shift = np.where(low, shift + np.log(np.where(low, y, 1)), shift)
        y = np.where(low, y + 1, y)
    i2 = 1 / (y * y)
    coef = [1 / dtype(12), -1 / dtype(360), 1 / dtype(1260), -1 / dtype(1680), 1 / dtype(1188), -dtype(691) / dtype(360360), 1 / dtype(156),
            -dtype(3617) / dtype(122400)]
    ser = np.zeros_like(y)
    for c in reversed(coef):
        ser = ser * i2 + c
    half_log_2pi = np.log(2 * np.arccos(dtype(-1))) / 2
    return (y - dtype(0.5)) * np.log(y) - y + half_log_2pi + ser / y - shift


def block(e, t, sample, seed, stream):
    """The four words (uint32 arrays) of round t for the uint64 element indices e of sample counter ``sample``."""
    e = np.asarray(e, dtype=np.uint64)
    c1 = (e >> np.uint64(32)) | np.uint64(int(t) << 20)
    return S.philox4x32_10([e & np.uint64(MASK), c1, np.full(e.shape, sample & MASK, dtype=np.uint64), np.full(e.shape, stream, dtype=np.uint64)],
                           (seed & MASK, seed >> 32))


def u01(r, dtype):
    return (r.astype(dtype) + dtype(0.5)) * dtype(2.0 ** -32)


def draw_plane(rate32, sample, seed, stream, dtype=np.float64, e0=0):
    """(k float64 [n] with NaN where the rate is refused, attempts int [n]: PTRS attempts used, 0 on the other branches, 65 where
    the bounded loop fell back to rint(rate)) for the float32 rates of one sample; element i has index e0 + i."""
    rate32 = np.asarray(rate32, dtype=np.float32).ravel()
    n = rate32.size
    e = np.arange(n, dtype=np.uint64) + np.uint64(e0)
    rate = rate32.astype(dtype)
    k = np.zeros(n, dtype=np.float64)
    attempts = np.zeros(n, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        bad = ~(rate >= 0) | (rate > dtype(RATE_MAX))
        small = ~bad & (rate < dtype(SMALL))
        big = ~bad & ~small
    k[bad] = np.nan
    # ---- inversion
    idx = np.flatnonzero(small)
    if idx.size:
        lam = rate[idx]
        u = u01(block(e[idx], 0, sample, seed, stream)[0], dtype)
        kk = np.zeros(idx.size, dtype=np.int64)
        p = np.exp(-lam)
        F = p.copy()
        for _ in range(MAX_STEPS):
            go = (u > F) & (kk < MAX_STEPS)
            if not go.any():
                break
            kk = np.where(go, kk + 1, kk)
            p = np.where(go, p * (lam / np.maximum(kk, 1).astype(dtype)), p)
            F = np.where(go, F + p, F)
        k[idx] = kk
    # ---- PTRS
    idx = np.flatnonzero(big)
    if idx.size:
        lam = rate[idx]
        slam, loglam = np.sqrt(lam), np.log(lam)
        b = dtype(0.931) + dtype(2.53) * slam
        a = dtype(-0.059) + dtype(0.02483) * b
        inv_alpha = dtype(1.1239) + dtype(1.1328) / (b - dtype(3.4))
        vr = dtype(0.9277) - dtype(3.6224) / (b - dtype(2.0))
        res = np.rint(lam).astype(np.float64)                              # the fallback of the bounded loop
        att = np.full(idx.size, 2 * MAX_ROUNDS + 1, dtype=np.int64)
        live = np.arange(idx.size)
        for j in range(2 * MAX_ROUNDS):
            if not live.size:
                break
            if j % 2 == 0:
                w = block(e[idx[live]], j >> 1, sample, seed, stream)
            else:
                w = [v[keep_prev] for v in w]
            U = u01(w[2 * (j & 1)], dtype) - dtype(0.5)
            V = u01(w[2 * (j & 1) + 1], dtype)
            l, bb, aa = lam[live], b[live], a[live]
            us = dtype(0.5) - np.abs(U)
            kf = np.floor((dtype(2.0) * aa / us + bb) * U + l + dtype(0.43))
            accept = (us >= dtype(0.07)) & (V <= vr[live])
            reject = ~accept & ((kf < 0) | ((us < dtype(0.013)) & (V > us)))
            test = ~accept & ~reject
            if test.any():
                ti = np.flatnonzero(test)
                lhs = np.log(V[ti]) + np.log(inv_alpha[live][ti]) - np.log(aa[ti] / (us[ti] * us[ti]) + bb[ti])
                rhs = -l[ti] + kf[ti] * loglam[live][ti] - lgamma(kf[ti] + 1, dtype)
                accept[ti] = lhs <= rhs
            done = live[accept]
            res[done] = kf[accept].astype(np.float64)
            att[done] = j + 1
            keep_prev = ~accept
            live = live[keep_prev]
        k[idx] = res
        attempts[idx] = att
    return k, attempts


def ptrs_proposal(rate32, e, j, sample, seed, stream, dtype=np.float64):
    """The k that attempt j (0-based) of the PTRS loop proposes for element e at the float32 rate (accepted or not)."""
    lam = dtype(np.float32(rate32))
    w = block(np.array([e], dtype=np.uint64), j >> 1, sample, seed, stream)
    U = u01(w[2 * (j & 1)], dtype)[0] - dtype(0.5)
    b = dtype(0.931) + dtype(2.53) * np.sqrt(lam)
    a = dtype(-0.059) + dtype(0.02483) * b
    return float(np.floor((dtype(2.0) * a / (dtype(0.5) - abs(U)) + b) * U + lam + dtype(0.43)))


def rand_poisson(lam, seed, stream=0, sample_offset=0, n_samples=None, pre=None, post=None, dtype=np.float64, return_attempts=False):
    """float32 array shaped like ops.rand_poisson's result.  lam float32; ``pre`` / ``post``: None, a number or [N]."""
    lam = np.asarray(lam, dtype=np.float32)
    if n_samples is None:
        N, planes, shape = lam.shape[0], lam.reshape(lam.shape[0], -1), lam.shape
    else:
        N, planes, shape = int(n_samples), None, (int(n_samples),) + lam.shape
    pre = None if pre is None else np.broadcast_to(np.asarray(pre, dtype=np.float32), (N,))
    post = None if post is None else np.broadcast_to(np.asarray(post, dtype=np.float32), (N,))
    out = np.empty((N, lam.size if n_samples is not None else planes.shape[1]), dtype=np.float32)
    att = np.empty(out.shape, dtype=np.int64)
    for s in range(N):
        rate = lam.ravel() if planes is None else planes[s]
        if pre is not None:
            with np.errstate(invalid="ignore", over="ignore"):
                rate = rate * pre[s]                                       # float32 * float32 -> float32
        k, att[s] = draw_plane(rate, sample_offset + s, seed, stream, dtype)
        k32 = k.astype(np.float32)
        out[s] = k32 if post is None else k32 * post[s]
    return (out.reshape(shape), att.reshape(shape)) if return_attempts else out.reshape(shape)


def mixed_rates(n, rng):
    """The mixed-rate input of the tests: quarters uniform in (0, 10), (10, 100), (100, 1100) and (1000, 70000), shuffled."""
    q = n // 4
    lam = np.concatenate([rng.uniform(0, 10, q), rng.uniform(10, 100, q), rng.uniform(100, 1100, q), rng.uniform(1000, 70000, n - 3 * q)])
    rng.shuffle(lam)
    return lam.astype(np.float32)
