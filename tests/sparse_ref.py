"""The numpy restatement of sparse-activity extraction, test infrastructure only: the order-preserving keys, the
per-pixel selection as a sort of the keys along time AND as the bisection the kernels run, the float64 frame dots, the residual in
numpy float32 operations in the library's order, ``extract_sparse`` end to end, and the scenes the tests share."""
import math
from collections import namedtuple

import numpy as np

SparseSplit = namedtuple("SparseSplit", ["sparse", "baseline", "scales", "tau"])
f32 = np.float32


# ------------------------------------------------------------------------------------------------ keys
def key32(v):
    """uint32 keys of float32 values: the unsigned image of the bits of v + 0.0f (-0 and +0 are one value) that orders like v."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey32(k):
    k = np.asarray(k, dtype=np.uint32)
    pos = (k & np.uint32(0x80000000)) != 0
    return np.where(pos, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def key16(h):
    """uint16 keys of float16 values, the same construction on 16 bits."""
    u = np.ascontiguousarray(h, dtype=np.float16).view(np.uint16).copy()
    u[(u & np.uint16(0x7FFF)) == 0] = 0
    neg = (u & np.uint16(0x8000)) != 0
    return np.where(neg, ~u, u | np.uint16(0x8000)).astype(np.uint16)


def unkey16(k):
    k = np.asarray(k, dtype=np.uint16)
    pos = (k & np.uint16(0x8000)) != 0
    return np.where(pos, k & np.uint16(0x7FFF), ~k).astype(np.uint16).view(np.float16)


# ------------------------------------------------------------------------------------------------ selection
def series(x, a=None, b=None):
    """The float32 series [T, P] the selection orders: x widened, minus fl32(a[t] * b[p]) where a background is given."""
    v = np.asarray(x).reshape(x.shape[0], -1).astype(np.float32)
    if a is not None:
        v = v - (np.asarray(a, dtype=f32)[:, None] * np.asarray(b, dtype=f32).reshape(1, -1))
        assert v.dtype == np.float32
    return v


def select_sort(keys, ranks):
    return np.sort(keys, axis=0)[list(ranks)]


def select_bisect(keys, ranks, bits):
    """What the kernels do: from the top bit down, the r-th smallest is >= prefix | bit iff fewer than r + 1 keys lie below it."""
    keys = keys.astype(np.uint64)
    out = []
    for r in ranks:
        prefix = np.zeros(keys.shape[1], dtype=np.uint64)
        for bit in range(bits - 1, -1, -1):
            cand = prefix | np.uint64(1 << bit)
            below = (keys < cand[None, :]).sum(axis=0)
            prefix = np.where(below <= r, cand, prefix)
        out.append(prefix)
    return np.stack(out)


def select(x, ranks, a=None, b=None):
    """float32 [K, P]: the ranks[k]-th smallest value of every pixel's series -- an element of it, with a zero returned as +0.  An
    fp16 stack without a background is ordered on 16-bit keys (the same order: widening is monotonic and exact)."""
    x = np.asarray(x)
    if x.dtype == np.float16 and a is None:
        return unkey16(select_sort(key16(x.reshape(x.shape[0], -1)), ranks)).astype(np.float32)
    return unkey32(select_sort(key32(series(x, a, b)), ranks))


def quantile_rank(q, n):
    return int(math.floor((n - 1) * float(q)))


# ------------------------------------------------------------------------------------------------ dots, residual, the pipeline
def frame_dots(x, b):
    """float64 [T + 1]: <x[t], b> and <b, b>, products and sums in float64 (numpy's order: exact only where every partial sum is)."""
    v = np.asarray(x).reshape(x.shape[0], -1).astype(np.float64)
    bb = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.concatenate([v @ bb, [bb @ bb]])


def residual(x, a, b, tau=None, pair=False):
    """S = relu(fl32(fl32(x - fl32(a * b)) - tau)), float32, the shape of x (plus a last axis (x, S) for ``pair``)."""
    r = series(x, a, b)
    if tau is not None:
        r = r - np.asarray(tau, dtype=f32).reshape(1, -1)
    s = np.where(r > 0, r, f32(0)).astype(np.float32).reshape(x.shape)
    return np.stack([np.asarray(x).astype(np.float32), s], axis=-1) if pair else s


def extract_sparse(frames, baseline_q=0.5, noise_k=0.0, ths=0.0, scale="ls", pair=False):
    N = frames.shape[0]
    baseline = select(frames, [quantile_rank(baseline_q, N)])[0]
    if scale == "ls":
        sums = frame_dots(frames, baseline)
        scales = (np.zeros(N) if sums[N] == 0 else sums[:N] / sums[N]).astype(np.float32)
    else:
        scales = np.ones(N, dtype=np.float32)
    if noise_k != 0:
        m, lo = select(frames, [quantile_rank(0.5, N), quantile_rank(0.1587, N)], scales, baseline)
        tau = (m + f32(noise_k) * (m - lo)) + f32(ths)
        assert tau.dtype == np.float32
    else:
        tau = np.full_like(baseline, ths) if ths != 0 else None
    s = residual(frames, scales, baseline, tau, pair)
    shape = frames.shape[1:]
    return SparseSplit(s, baseline.reshape(shape), scales, None if tau is None else tau.reshape(shape))


# ------------------------------------------------------------------------------------------------ scenes
Scene = namedtuple("Scene", ["frames", "bleach", "support", "signal"])


def scene(seed=0, T=120, H=48, W=48, blobs=12):
    """The planted scene: a Gaussian-bump background of 200 .. 1000 counts that bleaches from 1.0 to 0.74, ``blobs`` neurons with
    decaying transients, Poisson noise.  ``support``: the pixels a neuron touches; ``signal``: the noiseless transients."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    bg = 200.0 + 800.0 * np.exp(-((yy - H / 2) ** 2 + (xx - W / 2) ** 2) / (2 * (H / 3.0) ** 2))
    t = np.arange(T, dtype=np.float64)
    bleach = 1.0 - 0.26 * (1.0 - np.exp(-3.0 * t / max(T - 1, 1))) / (1.0 - math.exp(-3.0))
    signal = np.zeros((T, H, W))
    support = np.zeros((H, W), dtype=bool)
    for _ in range(blobs):
        cy, cx = rng.uniform(5, H - 5), rng.uniform(5, W - 5)
        prof = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 1.5 ** 2))
        trace = np.zeros(T)
        for t0 in rng.integers(5, T - 10, size=rng.integers(2, 5)):
            trace[t0:] += rng.uniform(150.0, 400.0) * np.exp(-(t[t0:] - t0) / 8.0)
        signal += trace[:, None, None] * prof[None]
        support |= prof > 1e-3
    clean = bg[None] * bleach[:, None, None] + signal
    return Scene(rng.poisson(clean).astype(np.float32), bleach, support, signal)


def grid_scene(seed=0, T=21, H=9, W=14, dtype=np.float32):
    """Small integers (exact in fp16, every float64 sum of products below 2^53 exact in any order): the whole pipeline's result is
    determined bit for bit.  A stepped background that fades over time, a few bright transients, a dead (all zero) pixel."""
    rng = np.random.default_rng(seed)
    bg = rng.integers(8, 40, size=(H, W))
    fade = np.linspace(8, 6, T).round().astype(np.int64)                       # eighths
    x = bg[None] * fade[:, None, None] // 8 + rng.integers(0, 6, size=(T, H, W))
    for _ in range(6):
        t0, y, c = rng.integers(0, T - 3), rng.integers(0, H), rng.integers(0, W)
        x[t0:t0 + 3, y, c] += rng.integers(30, 90)
    x[:, 0, 0] = 0
    return x.astype(dtype)
