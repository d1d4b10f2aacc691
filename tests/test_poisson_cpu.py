"""CPU: the Poisson draw of cwfa_rand_poisson_f32 as restated in poisson_ref.py -- is the scheme a Poisson
sampler, is float64 enough to decide every draw, does the bounded loop have margin, and do the counters chunk.  The GPU test
(test_gpu_poisson.py) then holds the kernel to this restatement element by element.  Also the host arithmetic of
``add_random_shot_noise_to_dataset`` on CPU tensors."""
import math

import numpy as np
import pytest
import torch

import poisson_ref as P

SEED = 0x5EED_C0FFEE            # fixed: the draw is a pure function of it, and the restatement passes every check below under it
N_DIST = 1 << 18
RATES = [0.05, 3.7, 9.999, 10.0, 37.5, 1024.0]


def log_pmf(k, rate):
    return -rate + k * math.log(rate) - np.array([math.lgamma(v + 1.0) for v in k])


def chi_square_p(k, rate):
    """p-value of Pearson's chi-square of the counts of k against Poisson(rate), tail bins merged to an expected count >= 5."""
    from scipy.stats import chi2
    n = k.size
    hi = int(rate + 12 * math.sqrt(rate) + 30)
    ks = np.arange(hi + 1, dtype=np.float64)
    expect = n * np.exp(log_pmf(ks, rate))
    counts = np.bincount(np.minimum(k.astype(np.int64), hi), minlength=hi + 1).astype(np.float64)
    expect[-1] += n - expect.sum()                                         # the tail beyond hi
    # the pmf is unimodal: the bins below 5 are a run at each end; each run becomes one bin, grown until it holds 5 itself
    lo_i = int(np.argmax(expect >= 5)) - 1 if expect[0] < 5 else 0
    while expect[:lo_i + 1].sum() < 5:
        lo_i += 1
    hi_i = hi - int(np.argmax(expect[::-1] >= 5)) + 1 if expect[-1] < 5 else hi
    while expect[hi_i:].sum() < 5:
        hi_i -= 1
    e = np.concatenate([[expect[:lo_i + 1].sum()], expect[lo_i + 1:hi_i], [expect[hi_i:].sum()]])
    c = np.concatenate([[counts[:lo_i + 1].sum()], counts[lo_i + 1:hi_i], [counts[hi_i:].sum()]])
    assert e.min() >= 5 and abs(e.sum() - n) < 1e-6 * n and c.sum() == n
    stat = ((c - e) ** 2 / e).sum()
    return float(chi2.sf(stat, e.size - 1)), stat, e.size - 1


@pytest.mark.parametrize("rate", RATES)
def test_the_draw_is_poisson(rate):
    lam = np.full((1, N_DIST), rate, dtype=np.float32)
    k = P.rand_poisson(lam, SEED).ravel().astype(np.float64)
    r = float(np.float32(rate))                                            # the rate the draw sees
    assert np.array_equal(k, np.rint(k)) and k.min() >= 0
    p, stat, dof = chi_square_p(k, r)
    mean, var = k.mean(), k.var(ddof=1)
    print(f"rate {rate}: chi2 {stat:.1f} / {dof} dof, p = {p:.4f}; mean - rate = {mean - r:+.3e} (bound {5 * math.sqrt(r / N_DIST):.3e}); "
          f"var / rate - 1 = {var / r - 1:+.3e} (bound {5 * math.sqrt(2 / N_DIST):.3e})")
    assert p > 1e-4
    assert abs(mean - r) <= 5 * math.sqrt(r / N_DIST)
    assert abs(var / r - 1) <= 5 * math.sqrt(2 / N_DIST)


@pytest.fixture(scope="module")
def mixed():
    lam = P.mixed_rates(1 << 18, np.random.default_rng(7))[None]
    k64, att = P.rand_poisson(lam, SEED, return_attempts=True)
    return lam, k64, att


def test_float64_decides_every_draw_as_longdouble_does(mixed):
    if np.finfo(np.longdouble).nmant <= np.finfo(np.float64).nmant:
        pytest.skip("numpy.longdouble is float64 on this platform")
    lam, k64, att64 = mixed
    kld, attld = P.rand_poisson(lam, SEED, dtype=np.longdouble, return_attempts=True)
    differ = int((k64 != kld).sum())
    print(f"float64 vs longdouble: {differ} of {k64.size} draws differ, attempts differ in {int((att64 != attld).sum())}")
    assert differ == 0 and np.array_equal(att64, attld)


def test_the_bounded_loop_has_margin(mixed):
    lam, _, att = mixed
    big = att[lam >= 10]
    hist = np.bincount(big)
    print(f"PTRS attempts: max {big.max()}, mean {big.mean():.3f}, histogram {hist.tolist()}")
    assert big.min() >= 1 and big.max() <= 16
    assert (att[lam < 10] == 0).all()


def test_chunks_streams_and_seeds():
    rng = np.random.default_rng(3)
    lam = P.mixed_rates(5 * 1031, rng).reshape(5, 1031)
    whole = P.rand_poisson(lam, SEED, stream=2, sample_offset=7)
    for cut in (1, 2, 4):
        parts = np.concatenate([P.rand_poisson(lam[:cut], SEED, stream=2, sample_offset=7),
                                P.rand_poisson(lam[cut:], SEED, stream=2, sample_offset=7 + cut)])
        assert np.array_equal(whole, parts)
    assert np.array_equal(whole, P.rand_poisson(lam, SEED, stream=2, sample_offset=7)), "a pure function of its arguments"
    assert (whole != P.rand_poisson(lam, SEED, stream=3, sample_offset=7)).mean() > 0.5
    assert (whole != P.rand_poisson(lam, SEED + 1, stream=2, sample_offset=7)).mean() > 0.5
    assert (whole != P.rand_poisson(lam, SEED + (1 << 32), stream=2, sample_offset=7)).mean() > 0.5, "the high half of the seed is key"
    shared = P.rand_poisson(lam[0], SEED, n_samples=3)
    assert shared.shape == (3, 1031) and np.array_equal(shared[2], P.rand_poisson(lam[:1], SEED, sample_offset=2)[0])
    assert (shared[0] != shared[1]).mean() > 0.5


def test_the_edges_of_the_rate():
    lam = np.array([[0.0, -0.0, -1.0, np.nan, 2.0 ** 30, np.nextafter(np.float32(2.0 ** 30), np.float32(np.inf)), np.inf, -np.inf,
                     np.float32(1e-30)]], dtype=np.float32)
    k = P.rand_poisson(lam, SEED)[0]
    assert k[0] == 0 and k[1] == 0 and k[8] == 0
    assert np.isnan(k[[2, 3, 5, 6, 7]]).all()
    assert abs(k[4] - 2.0 ** 30) < 12 * 2.0 ** 15                          # 12 standard deviations
    # pre and post: the draw at fl32(lam * pre), then fl32(k * post); pre = 0 gives 0
    rng = np.random.default_rng(5)
    lam = P.mixed_rates(2 * 515, rng).reshape(2, 515)
    pre, post = np.array([0.37, 2.5], dtype=np.float32), np.array([3.0, 0.1], dtype=np.float32)
    got = P.rand_poisson(lam, SEED, pre=pre, post=post)
    plain = P.rand_poisson(lam * pre[:, None], SEED)
    assert np.array_equal(got, plain * post[:, None])
    assert not P.rand_poisson(lam, SEED, pre=0.0).any()


def test_shot_noise_scales_match_their_restatement():
    from cwfa_amd.XLFMDataset import shot_noise_scales
    m = torch.tensor([3.5, 0.0, 1200.0, -2.0, 1e-20], dtype=torch.float32)
    u = torch.tensor([0.25, 0.5, 0.999, 0.1, 0.75], dtype=torch.float32)
    lo, hi = 16.0 ** 2, 64.0 ** 2
    pre, post = shot_noise_scales(m, u, [lo, hi])
    assert pre.dtype == post.dtype == torch.float32
    for i in range(m.numel()):
        if float(m[i]) <= 0:
            assert float(pre[i]) == 0 and float(post[i]) == 0
        else:
            Pw = torch.tensor(lo) + torch.tensor(hi - lo) * u[i]          # fp32, in the order the method documents
            assert float(pre[i]) == float(Pw / m[i]) and float(post[i]) == float(m[i] / Pw)
    same, _ = shot_noise_scales(m, u, [1024, 1024])
    assert float(same[0]) == float(torch.tensor(1024.0) / m[0])
    for bad in ([0, 10], [-1, 4], [8, 4], [1, float("inf")]):
        with pytest.raises(ValueError):
            shot_noise_scales(m, u, bad)
