"""Restatements for the sampler tests (CPU, numpy + torch): Philox4x32-10 with the counter convention of include/cwfa_hip.h, the
uniform map and the truncated-normal map of cwfa_rand_trunc_normal_f32 in float64.

Element e (contiguous linear index within ONE sample) of sample n takes word e & 3 of the block with counter
(g & 0xffffffff, g >> 32, sample_offset + n, stream_id), g = e >> 2, under the key (seed & 0xffffffff, seed >> 32)."""
import math

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two; returns the four output words as uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)                 # < 2^64: exact in uint64
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & MASK, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def words(N, n, seed, stream=0, sample_offset=0):
    """uint32 [N, n]: the word of element e of sample i."""
    e = np.arange(n, dtype=np.uint64)
    g = e >> np.uint64(2)
    out = np.empty((N, n), dtype=np.uint32)
    for i in range(N):
        blk = philox4x32_10([g & MASK, g >> np.uint64(32), np.full(n, (sample_offset + i) & MASK, dtype=np.uint64), np.full(n, stream, dtype=np.uint64)],
                            (seed & MASK, seed >> 32))
        out[i] = np.stack(blk, 1)[np.arange(n), (e & np.uint64(3)).astype(np.int64)]
    return out


def uniform_of(r):
    """u = ((r >> 9) + 0.5) * 2^-23, every step in float32 (each is exact)."""
    return ((r >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def uniform(N, n, seed, stream=0, sample_offset=0):
    return uniform_of(words(N, n, seed, stream, sample_offset))


def E_of(T):
    return np.float32(math.erf(T / math.sqrt(2.0)))


def trunc_normal_of(u, T):
    """float64: clamp(sqrt 2 * erfinv(a), -T, T) at the fp32 argument a = fl(E * fl(2u - 1)) the kernel forms."""
    a = E_of(T) * (np.float32(2.0) * u.astype(np.float32) - np.float32(1.0))
    assert a.dtype == np.float32
    z = math.sqrt(2.0) * torch.erfinv(torch.from_numpy(a.astype(np.float64)))
    return z.clamp(-T, T).numpy()


def trunc_normal(N, n, T, seed, stream=0, sample_offset=0):
    return trunc_normal_of(uniform(N, n, seed, stream, sample_offset), T)
