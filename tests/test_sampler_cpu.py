"""CPU: the sampler without a GPU -- the numpy restatement of the generator (tests/sampler_ref.py) against the Random123 known
answers of Philox4x32-10, the uniform map's exactness, the statistics of the truncated-normal map under the counter convention, and
the argument validation of cwfa_rand_uniform_f32 / cwfa_rand_trunc_normal_f32 / cwfa_chain_inv_samples_f32 through the built
library (no launch happens: every call below is refused, or empty)."""
import ctypes
import math

import numpy as np
import pytest

import sampler_ref as S

KAT = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.fixture(scope="module")
def L():
    from cwfa_amd import _lib, build
    build.build_all()
    return _lib.lib()


@pytest.fixture(scope="module")
def ptr():
    buf = ctypes.create_string_buffer(4096)
    return ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert " ".join(f"{int(v):08x}" for v in S.philox4x32_10(ctr, key)) == want


def test_counter_convention():
    """element e takes word e & 3 of block e >> 2; the sample counter is sample_offset + n; the key is the seed's two halves"""
    seed = (0xa4093822) | (0x299f31d0 << 32)
    w = S.words(2, 11, seed, stream=0x03707344, sample_offset=0x13198a2e - 1)
    blk = S.philox4x32_10([1, 0, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])
    assert [int(v) for v in w[1, 4:8]] == [int(v) for v in blk]
    assert np.array_equal(S.words(1, 11, seed, 0x03707344, 0x13198a2e)[0], w[1])
    assert not np.array_equal(w[0], w[1]) and not np.array_equal(S.words(1, 11, seed + 1, 0x03707344, 0x13198a2e)[0], w[1])


def test_uniform_is_exact_and_inside_the_open_interval():
    r = np.array([0, 1, 511, 512, 0x7fffffff, 0x80000000, 0xfffffdff, 0xfffffe00, 0xffffffff], dtype=np.uint32)
    r = np.concatenate([r, S.words(3, 1001, 12345)[1]])
    u = S.uniform_of(r)
    assert u.dtype == np.float32
    exact = ((r >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert np.array_equal(u.astype(np.float64), exact)                    # nothing was rounded
    assert u.min() == np.float32(2.0 ** -24) and u.max() == np.float32(1.0 - 2.0 ** -24) and 0.0 < u.min() and u.max() < 1.0
    # 2u - 1 is exact too: the argument of erfinv is one rounding (the product with E) away from the real number
    assert np.array_equal((np.float32(2.0) * u - np.float32(1.0)).astype(np.float64), 2.0 * exact - 1.0)


@pytest.mark.parametrize("T", [0.5, 1.0, 3.0, math.inf])
def test_truncated_normal_map(T):
    z = S.trunc_normal(1, 4096, T, 99)
    assert z.dtype == np.float64 and np.abs(z).max() <= T and np.abs(z).max() < 5.3
    assert np.abs(z).max() > 0.9 * min(T, 3.0)                             # the whole interval is reached
    # antisymmetric in u -> 1 - u, i.e. in the word r -> ~r
    r = S.words(1, 64, 7)
    assert np.array_equal(S.trunc_normal_of(S.uniform_of(~r), T), -S.trunc_normal_of(S.uniform_of(r), T))


def test_statistics_of_the_restatement():
    """seed 87, stream 0, samples 0 .. 255 of 1*3*24*64 elements at T = 1: the mean over the elements of (sample variance /
    z_var(1)) is 1.000778 and the largest |z-score| of the per-element means 3.60 -- inside the bounds the GPU test puts on the
    sampler (|r - 1| <= 7.8e-3, z-score < 6), and the figures the kernel's samples must show there (each latent used exactly once)."""
    from cwfa_amd import CWFA
    Sn, n = 256, 3 * 24 * 64
    z = S.trunc_normal(Sn, n, 1.0, 87)
    zv = CWFA.truncated_normal_variance(1)
    r = float((z.var(0, ddof=1) / zv).mean())
    zs = float(np.abs(z.mean(0) / math.sqrt(zv / Sn)).max())
    print(f"[sampler] restatement: r = {r:.6f}, largest z-score {zs:.2f}")
    assert abs(r - 1.000778) < 1e-6 and abs(zs - 3.60) < 5e-3
    assert abs(r - 1.0) <= 6.0 * math.sqrt(2.0 / ((Sn - 1) * n)) and zs < 6.0


def test_rand_arguments(L, ptr):
    p = ptr
    for fn, extra in ((L.cwfa_rand_uniform_f32, ()), (L.cwfa_rand_trunc_normal_f32, (1.0,))):
        name = b"cwfa_rand_uniform_f32" if not extra else b"cwfa_rand_trunc_normal_f32"
        assert fn(None, 1, 8, 8, *extra, 1, 0, 0, None) == -1 and name + b": null" in L.cwfa_last_error()
        assert fn(p, -1, 8, 8, *extra, 1, 0, 0, None) == -2 and fn(p, 1, -8, 8, *extra, 1, 0, 0, None) == -2
        assert fn(p, 2, 8, 7, *extra, 1, 0, 0, None) == -1 and b"sample stride" in L.cwfa_last_error()
        assert fn(p, 0, 8, 8, *extra, 1, 0, 0, None) == 0 and fn(p, 3, 0, 0, *extra, 1, 0, 0, None) == 0
    for T in (0.0, -1.0, float("nan"), -math.inf):
        assert L.cwfa_rand_trunc_normal_f32(p, 1, 8, 8, T, 1, 0, 0, None) == -1 and b"temperature" in L.cwfa_last_error(), T
    assert L.cwfa_rand_trunc_normal_f32(p, 0, 8, 8, math.inf, 1, 0, 0, None) == 0


def test_chain_inv_samples_arguments(L, ptr):
    from cwfa_amd import _lib
    p, q = ptr, ctypes.c_void_p(ptr.value + 1024)
    ch = _lib.Chain()
    ok = ctypes.byref(ch)

    def call(low=p, x=q, z=None, chain=ok, N=1, B=1, C=2, H=4, W=8, ss=(0, 64, 128, 128, 64, 64), T=1.0):
        return L.cwfa_chain_inv_samples_f32(low, x, z, chain, N, B, C, H, W, *ss, T, 3, 0, 0, None)
    assert call(low=None) == -1 and b"cwfa_chain_inv_samples_f32: null" in L.cwfa_last_error()
    assert call(x=None) == -1
    for bad in (dict(N=-1), dict(B=-1), dict(C=-1), dict(H=-1), dict(W=-1), dict(B=65536)):
        assert call(**bad) == -2 and b"bad shape" in L.cwfa_last_error(), bad
    assert call(chain=None) == -1 and b"null chain" in L.cwfa_last_error()
    for T in (0.0, -0.5, float("nan")):
        assert call(T=T) == -1 and b"temperature" in L.cwfa_last_error(), T
    assert call(ss=(-1, 64, 128, 128, 64, 64)) == -1 and b"stride" in L.cwfa_last_error()
    # strides that do not cover what they step over, and a z_out inside x
    assert call(B=2, ss=(0, 63, 128, 128, 64, 64)) == -1 and b"batch stride" in L.cwfa_last_error()
    assert call(B=2, ss=(0, 64, 128, 127, 64, 64)) == -1 and call(B=2, z=p, ss=(0, 64, 256, 128, 128, 63)) == -1
    assert call(N=2, ss=(0, 64, 127, 128, 64, 64)) == -1 and b"sample stride" in L.cwfa_last_error()
    assert call(N=2, ss=(63, 64, 128, 128, 64, 64)) == -1 and call(N=2, z=p, ss=(0, 64, 128, 128, 63, 64)) == -1
    assert call(z=ctypes.c_void_p(q.value + 4 * 127)) == -1 and b"overlaps" in L.cwfa_last_error()
    assert call(z=ctypes.c_void_p(q.value - 4 * 63)) == -1 and b"overlaps" in L.cwfa_last_error()
    bad = _lib.Chain()
    bad.n_stages = _lib.CHAIN_MAX + 1
    assert call(chain=ctypes.byref(bad)) == -1 and b"stages" in L.cwfa_last_error()
    gin = _lib.Chain()
    gin.n_stages = 1
    gin.stage[0].gin = 1
    gin.stage[0].perm_axis = 1
    assert call(chain=ctypes.byref(gin)) == -1 and b"GIN" in L.cwfa_last_error()
    axis = _lib.Chain()
    axis.n_stages = 1
    axis.stage[0].perm = p.value
    axis.stage[0].perm_axis = 7
    assert call(chain=ctypes.byref(axis)) == -1
    # empty problems are accepted and do nothing (z_out is nullable)
    assert call(N=0) == 0 and call(B=0) == 0 and call(C=0) == 0 and call(T=math.inf, H=0) == 0


def test_python_wrappers_refuse_before_any_launch():
    import torch

    from cwfa_amd import CWFA, ops
    with pytest.raises(ValueError, match="temperature"):
        ops.chain_inv_samples(torch.zeros(1, 2, 4, 8), [], 2, 0.0, 1)
    with pytest.raises(ValueError, match="n_samples"):
        ops.chain_inv_samples(torch.zeros(1, 2, 4, 8), [], 0, 1.0, 1)
    with pytest.raises(ValueError, match="64-bit"):
        ops._rand_args(-1, 0, 0, "x")
    with pytest.raises(ValueError, match="32-bit"):
        ops._rand_args(1, 1 << 32, 0, "x")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.chain_inv_samples(torch.zeros(1, 2, 4, 8), [], 2, 1.0, 1)
    # temperature 0 needs no generator: zeros, with or without a seed
    assert not CWFA.sample_z_truncated((2, 3), "cpu", 0, seed=5).any()
