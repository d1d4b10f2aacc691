"""The numpy restatement of the trace post-processing: the 64-bit order, the sliding quantile, the row select,
the noise level, dF/F and the AR(1) deconvolution -- one float64 operation at a time, the deconvolution literally the listing of
section 28.1 -- and the scene the purpose tests share.  Test infrastructure: the product has no CPU path."""
import numpy as np

QNAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]
SIGMA_SCALE = 1.0483580825075305                                               # 1 / (0.6744897501960817 * sqrt(2))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def ordered(a):
    """The values of ``a`` in the order: np.sort (NaN last), -0 as +0, every NaN the canonical quiet NaN."""
    s = np.sort(np.asarray(a, dtype=np.float64), axis=-1) + 0.0
    s[np.isnan(s)] = QNAN
    return s


def sliding_quantile(x, h, p, at=None):
    """``at``: only these t (the columns of the result)."""
    x = np.asarray(x, dtype=np.float64)
    N, T = x.shape
    ts = range(T) if at is None else list(at)
    out = np.empty((N, len(ts)))
    for i, t in enumerate(ts):
        lo, hi = max(0, t - h), min(T - 1, t + h)
        out[:, i] = ordered(x[:, lo:hi + 1])[:, (p * (hi - lo)) // 100]
    return out


def trace_select(x, ranks):
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((len(ranks), x.shape[0]))
    for n in range(x.shape[0]):
        s = ordered(x[n])
        for k, r in enumerate(ranks):
            out[k, n] = s[r]
    return out


def lmed(a):
    """Per row the element of rank (len - 1) // 2."""
    return trace_select(a, [(a.shape[1] - 1) // 2])[0]


def trace_noise(x):
    x = np.asarray(x, dtype=np.float64)
    if x.shape[1] < 2:
        return np.full(x.shape[0], np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[:, 1:] - x[:, :-1]
        med = lmed(d)
        mad = lmed(np.abs(d - med[:, None]))
        return mad * SIGMA_SCALE


def delta_f_over_f(F, Fnp, alpha, h, p, floor=0.0):
    F = np.asarray(F, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        Fc = F if Fnp is None else np.where(np.isnan(Fnp), F, F - alpha * Fnp)
        B = sliding_quantile(Fc, h, p)
        D = B if Fnp is None else sliding_quantile(F, h, p)
        den = np.maximum(D, floor)
        dff = np.where(den > 0, (Fc - B) / np.where(den > 0, den, 1.0), np.nan)
    return dff, B, D


def powers(gamma, T):
    pw = np.empty(T + 1)
    pw[0] = 1.0
    for k in range(1, T + 1):
        pw[k] = pw[k - 1] * gamma
    return pw


def ar1_row(y, gamma, lam):
    """The listing of section 28.1 for one row: (c, s, number of pools)."""
    y = np.asarray(y, dtype=np.float64)
    T = len(y)
    gamma, lam = np.float64(gamma), np.float64(lam)
    if not np.isfinite(y).all() or not (lam >= 0.0 and lam < np.inf):
        return np.full(T, QNAN), np.full(T, QNAN), 0
    pw = powers(gamma, T)
    m = lam * (np.float64(1.0) - gamma)
    z = y - m
    z[T - 1] = y[T - 1] - lam
    V, W, S, L = [], [], [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(T):
            V.append(z[t]), W.append(np.float64(1.0)), S.append(t), L.append(1)
            while len(V) > 1 and V[-1] < pw[L[-2]] * V[-2]:
                a = pw[L[-2]]
                w = W[-2] + (a * a) * W[-1]
                v = (W[-2] * V[-2] + (a * W[-1]) * V[-1]) / w
                V[-2], W[-2], L[-2] = v, w, L[-2] + L[-1]
                V.pop(), W.pop(), S.pop(), L.pop()
        c, s = np.empty(T), np.zeros(T)
        vp = [v if v > 0.0 else np.float64(0.0) for v in V]
        for i in range(len(V)):
            for k in range(L[i]):
                c[S[i] + k] = pw[k] * vp[i]
            s[S[i]] = vp[0] if i == 0 else vp[i] - pw[L[i - 1]] * vp[i - 1]
    return c, s, len(V)


def ar1_deconv(y, gamma, lam):
    y = np.asarray(y, dtype=np.float64)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (y.shape[0],))
    c, s, pools = np.empty(y.shape), np.empty(y.shape), np.zeros(y.shape[0], dtype=np.int32)
    for n in range(y.shape[0]):
        c[n], s[n], pools[n] = ar1_row(y[n], gamma, lam[n])
    return c, s, pools


def infer_spikes(y, gamma, lam_sigma):
    with np.errstate(invalid="ignore"):
        lam = np.float64(lam_sigma) * trace_noise(y)
    return ar1_deconv(y, gamma, lam)


def ar1_response(s, gamma):
    c = np.empty(len(s))
    for t in range(len(s)):
        c[t] = s[t] if t == 0 else gamma * c[t - 1] + s[t]
    return c


# ------------------------------------------------------------------------------------------------ the scene
SCENE_N, SCENE_T, SCENE_GAMMA, SCENE_NOISE = 8, 600, 0.9, 0.1


def scene(seed):
    """(F [8,600], calcium c, spikes s): spikes with probability 0.03 per sample and amplitude 0.5 + U(0,1), c their AR(1) response
    (gamma = 0.9), base = (2 + 2U)(0.6 + 0.4 exp(-t/250))(1 + 0.1 sin(2 pi t / 400 + 6U)), F = base (1 + c) + 0.1 N(0,1)."""
    rng = np.random.default_rng(seed)
    N, T = SCENE_N, SCENE_T
    t = np.arange(T, dtype=np.float64)
    s = (rng.random((N, T)) < 0.03) * (0.5 + rng.random((N, T)))
    c = np.stack([ar1_response(s[n], SCENE_GAMMA) for n in range(N)])
    base = (2.0 + 2.0 * rng.random((N, 1))) * (0.6 + 0.4 * np.exp(-t / 250.0)) * (1.0 + 0.1 * np.sin(2.0 * np.pi * t / 400.0 + 6.0 * rng.random((N, 1))))
    F = base * (1.0 + c) + SCENE_NOISE * rng.standard_normal((N, T))
    return F, c, s


def corr_rows(a, b):
    return np.array([np.corrcoef(a[n], b[n])[0, 1] for n in range(a.shape[0])])


_PIPE = {}


def scene_pipeline(seed, h=75, p=10, lam_sigma=2.0):
    """The whole restated pipeline on ``scene(seed)``, computed once and shared: a dict of F, c, s and dff, B, sigma, cd, sd, pools."""
    key = (seed, h, p, lam_sigma)
    if key not in _PIPE:
        F, c, s = scene(seed)
        dff, B, _ = delta_f_over_f(F, None, 0.7, h, p)
        sigma = trace_noise(dff)
        cd, sd, pools = infer_spikes(dff, SCENE_GAMMA, lam_sigma)
        _PIPE[key] = dict(F=F, c=c, s=s, dff=dff, B=B, sigma=sigma, cd=cd, sd=sd, pools=pools)
    return _PIPE[key]


# ------------------------------------------------------------------------------------------------ value cases of the order
def value_rows(T, seed=0):
    """Rows of T samples that exercise the order: equal values, 4 levels, negatives, +-0, denormals, +-inf, NaNs of both signs at the
    ends and inside, all NaN, pairs that differ in the last mantissa bit, magnitudes from 1e-300 to 1e300."""
    rng = np.random.default_rng(seed)
    u = lambda: rng.standard_normal(T)
    neg_nan = np.array([0xfff8000000000001], dtype=np.uint64).view(np.float64)[0]
    rows = [np.full(T, 3.25), np.floor(rng.random(T) * 4.0) / 4.0, -np.abs(u()) - 1.0, u()]
    z = np.where(rng.random(T) < 0.5, 0.0, -0.0)
    rows.append(z)
    rows.append(np.where(rng.random(T) < 0.3, u(), z))
    rows.append(rng.integers(-40, 40, T).astype(np.float64) * 4.9406564584124654e-324)
    r = u()
    r[rng.random(T) < 0.2] = np.inf
    r[rng.random(T) < 0.2] = -np.inf
    rows.append(r)
    r = u()
    r[0], r[-1] = np.nan, neg_nan
    r[T // 2] = neg_nan
    r[T // 3] = np.nan
    rows.append(r)
    r = u()
    r[rng.random(T) < 0.6] = np.nan
    r[: min(T, 9)] = neg_nan                                                       # an all-NaN window at the start
    rows.append(r)
    rows.append(np.full(T, np.nan))
    base = bits(1.0 + rng.integers(0, 3, T) * 2.0 ** -30).copy()
    rows.append((base + rng.integers(0, 2, T).astype(np.uint64)).view(np.float64) * np.where(rng.random(T) < 0.5, 1.0, -1.0))
    rows.append(np.sign(u()) * 10.0 ** rng.uniform(-300, 300, T))
    return np.stack(rows)
