"""The numpy restatement of the neuron detector and the scene the end-to-end tests plant neurons in.  No test
functions here; tests/test_neurons_cpu.py and tests/test_gpu_neurons.py import it.

    key(v) = ord(S[v]) << 32 | (0xFFFFFFFF - lin(v))
    v is a peak  <=>  S[v] is not NaN, S[v] >= thr, v is at least `margin` from every face, and key(v) is the maximum of the keys
                      over the box of half-widths `dist` around v, clipped by the volume

ord: the order-preserving unsigned image of the fp32 bits of S + 0.0 (so -0 and +0 are one value), NaN -> 0; lin: the linear index."""
import functools

import numpy as np


def ord32(s):
    s = np.asarray(s, dtype=np.float32) + np.float32(0.0)
    u = s.view(np.uint32)
    o = np.where(u >> np.uint32(31) == 1, ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(s), np.uint32(0), o).astype(np.uint32)


def keys(score):
    score = np.ascontiguousarray(score, dtype=np.float32)
    assert score.ndim == 3 and score.size <= 1 << 32
    lin = np.arange(score.size, dtype=np.uint64).reshape(score.shape)
    return (ord32(score).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - lin)


def window_max(k, dist):
    """The maximum of k over the box of half-widths dist, clipped by the volume: per axis, dist[axis] shifts each way."""
    for axis, d in enumerate(dist):
        out = k.copy()
        n = k.shape[axis]
        for s in range(1, min(int(d), n - 1) + 1 if n else 0):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, n - s), slice(s, n)
            lo, hi = tuple(lo), tuple(hi)
            out[lo] = np.maximum(out[lo], k[hi])
            out[hi] = np.maximum(out[hi], k[lo])
        k = out
    return k


def local_maxima(score, thr, dist, margin=(0, 0, 0), n_max=None):
    """(zyx int32 [K,3], scores float32 [K], total): the peaks by key descending, the first n_max of them."""
    score = np.ascontiguousarray(score, dtype=np.float32)
    D, H, W = score.shape
    k = keys(score)
    with np.errstate(invalid="ignore"):
        peak = (k == window_max(k, dist)) & ~np.isnan(score) & (score >= np.float32(thr))
    inside = np.zeros(score.shape, dtype=bool)
    mz, my, mx = (int(m) for m in margin)
    inside[mz:max(D - mz, mz), my:max(H - my, my), mx:max(W - mx, mx)] = True
    lin = np.flatnonzero(peak & inside)
    lin = lin[np.argsort(k.reshape(-1)[lin])[::-1]]
    total = len(lin)
    if n_max is not None:
        lin = lin[:n_max]
    zyx = np.stack([lin // (H * W), lin // W % H, lin % W], axis=1).astype(np.int32) if total else np.zeros((0, 3), dtype=np.int32)
    return zyx, score.reshape(-1)[lin], total


def far_apart(zyx, dist):
    """Every two rows differ by more than dist on at least one axis."""
    z = np.asarray(zyx, dtype=np.int64)
    gap = np.abs(z[:, None, :] - z[None, :, :]) > np.asarray(dist)[None, None, :]
    return bool((gap.any(-1) | np.eye(len(z), dtype=bool)).all())


def boxes_disjoint(boxes):
    """Half-open (z0, z1, y0, y1, x0, x1) boxes: every two are separated on at least one axis."""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 3, 2)
    apart = (b[:, None, :, 1] <= b[None, :, :, 0]) | (b[None, :, :, 1] <= b[:, None, :, 0])
    return bool((apart.any(-1) | np.eye(len(b), dtype=bool)).all())


@functools.lru_cache(maxsize=None)
def scene(seed, D=24, H=96, W=112, T=40, N=24):
    """(stack float32 [T,D,H,W], centres int [N,3] as (z, y, x)): N Gaussian blobs (sigma 1.2, 2, 2) whose centres differ pairwise by
    at least (12, 20, 20) on some axis, amplitude (0.5 + U(0,1)) (1 + i / 8) per time step and set to 0 with probability 0.6, plus
    0.01 U(0,1) noise on every voxel.  Shared by the tests that need it: do not write into the arrays."""
    rng = np.random.default_rng(seed)
    centres = []
    while len(centres) < N:
        c = (int(rng.integers(3, D - 3)), int(rng.integers(5, H - 5)), int(rng.integers(5, W - 5)))
        if all(abs(c[0] - o[0]) >= 12 or abs(c[1] - o[1]) >= 20 or abs(c[2] - o[2]) >= 20 for o in centres):
            centres.append(c)
    z, y, x = np.arange(D)[:, None, None], np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    stack = np.zeros((T, D, H, W), dtype=np.float64)
    for i, (cz, cy, cx) in enumerate(centres):
        blob = np.exp(-0.5 * (((z - cz) / 1.2) ** 2 + ((y - cy) / 2.0) ** 2 + ((x - cx) / 2.0) ** 2))
        amp = (0.5 + rng.random(T)) * (1 + i / 8)
        amp[rng.random(T) < 0.6] = 0.0
        stack += amp[:, None, None, None] * blob[None]
    stack += 0.01 * rng.random(stack.shape)
    stack = stack.astype(np.float32)
    stack.setflags(write=False)
    centres = np.array(centres, dtype=np.int64)
    centres.setflags(write=False)
    return stack, centres
