"""CPU: the likelihood maps without a GPU -- the algebra of cwfa_chain_nll_map_f32 / cwfa_nll_compose_f32 in
float64 against the existing restatements of the chain (tests/chain_ref.py), and the argument validation of both entry points
through the built library (no launch happens: every call below is refused, or empty)."""
import ctypes
import math

import pytest
import torch

import chain_ref as CR
import nllmap_ref as R

SHAPE, AXES = (2, 3, 5, 7), [3, 1, None, 2, 3, 1]
KINDS = dict(no_s=(4,), no_t=(1,), kinds=["NONE", "ATAN", "TANH", "SIGMOID", "ATAN", "TANH"], pres=[1.0, 1.0, 0.1, 1.0, 1.0, 1.0],
             clamps=[0.5, 2.0, 2.0, 1.5, 2.0, 1.0])


def _x(shape, seed):
    B, C, H, W = shape
    return torch.randn((B, 2 * C, H, W), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("kw", [{}, KINDS], ids=["atan", "kinds"])
def test_identities(kw):
    """(1) a sample's map sums to 0.5 * sum z^2 - logdet of the forward chain; (2) the forward chain's z, read where each volume
    position's latent starts, is the map's z -- and its magnitude walk the map's error scale; (3) z of a volume built by the inverse
    chain from given latents is those latents."""
    stages = R.random_stages(SHAPE, AXES, 11, **kw)
    x = _x(SHAPE, 12)
    m = R.chain_nll_map(x, stages)
    fwd = CR.inverse_stages(stages)
    z, low, logdet, sumsq = CR.chain_fwd(x, fwd)
    want = 0.5 * (z * z).flatten(1).sum(1) - logdet
    assert float((m["nll_sum"] - want).abs().max()) < 1e-10
    assert abs(float(m["nll_sum"].sum()) - (0.5 * sumsq - float(logdet.sum()))) < 1e-10
    assert float((R.at_positions(z, stages) - m["z"]).abs().max()) < 1e-10
    assert float((low - m["low"]).abs().max()) == 0.0
    M = R.at_positions(CR.chain_magnitude(fwd, x=x), stages)
    assert float(((M - m["M"]).abs() / M).max()) < 1e-10
    # the volume of given latents: z-scores = the latents at the positions they arrive at
    zs = torch.randn(SHAPE, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    xs, _ = CR.chain_inv(zs, low, stages)
    back = R.chain_nll_map(xs, stages)
    assert float((back["z"] - R.at_positions(zs, stages)).abs().max()) < 1e-10
    assert float((back["low"] - low).abs().max()) < 1e-10


def test_compose():
    """D = 16, L = 3: every depth takes 2^-(n+1) of the coefficient above it, the total is the total of the levels, and the fp32
    expression has exact products (it equals the float64 one wherever the sums are exact)."""
    g = torch.Generator().manual_seed(14)
    levels = [torch.randn(2, 16 >> (n + 1), 3, 5, generator=g) for n in range(3)]
    out = R.compose(levels)
    assert out.shape == (2, 16, 3, 5)
    for d in range(16):
        want = sum(levels[n][:, d >> (n + 1)].double() * 0.5 ** (n + 1) for n in range(3))
        assert torch.equal(out[:, d], want)
    tot = sum(lv.double().flatten(1).sum(1) for lv in levels)
    assert float((out.flatten(1).sum(1) - tot).abs().max()) < 1e-10
    ints = [torch.randint(-8, 9, lv.shape, generator=g).float() for lv in levels]       # small integers: nothing rounds in fp32
    assert torch.equal(R.compose(ints, torch.float32).double(), R.compose(ints))
    assert R.compose(levels, torch.float32).dtype == torch.float32


def test_coverage_seed_on_the_restatement():
    """The draws the GPU test's coverage case sees (8 samples of 1 x 3 x 24 x 64 at T = inf, stream 0), from the numpy restatement of
    the generator: inside 6 sqrt(p (1 - p) / N) of erf(k / sqrt 2) for the chosen seed, with room to spare."""
    import sampler_ref as S
    from cwfa_amd import CWFA
    n = math.prod(R.POS_SHAPE)
    z = torch.from_numpy(S.trunc_normal(8, n, math.inf, R.POS_SEED))
    assert z.numel() == 36864
    obs, exp = CWFA.zscore_coverage([z])
    for o, p in zip(obs[0].tolist(), exp.tolist()):
        band = 6.0 * math.sqrt(p * (1.0 - p) / z.numel())
        print(f"[nllmap] restatement coverage {o:.5f} (normal {p:.5f}, band {band:.5f})")
        assert abs(o - p) <= 0.5 * band


@pytest.fixture(scope="module")
def L():
    from cwfa_amd import _lib, build
    build.build_all()
    return _lib.lib()


@pytest.fixture(scope="module")
def ptr():
    buf = ctypes.create_string_buffer(8192)
    return ctypes.cast(buf, ctypes.c_void_p)


def test_chain_nll_map_arguments(L, ptr):
    from cwfa_amd import _lib
    p = ptr
    q, r, s, acc = (ctypes.c_void_p(ptr.value + 1024 * k) for k in (1, 2, 3, 4))
    ch = _lib.Chain()
    ok = ctypes.byref(ch)

    def call(x=p, low=q, z=r, nll=s, chain=ok, B=0, C=2, H=4, W=8, bs=(128, 64, 64, 64), nll_sum=acc):
        return L.cwfa_chain_nll_map_f32(x, low, z, nll, chain, B, C, H, W, *bs, nll_sum, None)
    assert call(x=None) == -1 and b"cwfa_chain_nll_map_f32: null" in L.cwfa_last_error()
    assert call(low=None, z=None, nll=None, nll_sum=None) == -1 and b"no output" in L.cwfa_last_error()
    for keep in ("low", "z", "nll", "nll_sum"):                      # any one output is enough
        assert call(**{k: None for k in ("low", "z", "nll", "nll_sum") if k != keep}) == 0, keep
    for bad in (dict(B=-1), dict(C=-1), dict(H=-1), dict(W=-1), dict(B=65536)):
        assert call(**bad) == -2 and b"bad shape" in L.cwfa_last_error(), bad
    assert call(chain=None) == -1 and b"null chain" in L.cwfa_last_error()
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
    # batch strides that do not cover a batch entry (checked before any launch)
    for bs in ((127, 64, 64, 64), (128, 63, 64, 64), (128, 64, 63, 64), (128, 64, 64, 63)):
        assert call(B=2, bs=bs) == -1 and b"batch stride" in L.cwfa_last_error(), bs
    # empty problems are accepted and do nothing
    assert call(B=0) == 0 and call(B=3, C=0) == 0 and call(B=3, H=0) == 0 and call(B=3, W=0) == 0


def test_nll_compose_arguments(L, ptr):
    from cwfa_amd import _lib
    p, out = ptr, ctypes.c_void_p(ptr.value + 4096)

    def table(n, null_at=None, bs=64):
        t = _lib.NllLevels()
        t.n = n
        for k in range(min(n, _lib.NLL_MAX_LEVELS)):
            t.level[k] = None if k == null_at else p.value
            t.bs[k] = bs
        return t

    def call(tab=None, o=out, B=0, D=16, HW=4, obs=64):
        return L.cwfa_nll_compose_f32(ctypes.byref(tab if tab is not None else table(3)), o, B, D, HW, obs, None)
    assert L.cwfa_nll_compose_f32(None, out, 0, 16, 4, 64, None) == -1 and b"cwfa_nll_compose_f32: null" in L.cwfa_last_error()
    assert call(o=None) == -1
    for n in (0, -1, _lib.NLL_MAX_LEVELS + 1):
        assert call(tab=table(n)) == -1 and b"levels" in L.cwfa_last_error(), n
    for bad in (dict(B=-1), dict(D=-1), dict(HW=-1), dict(B=65536), dict(D=65536 * 8)):
        assert call(**bad) == -2 and b"bad shape" in L.cwfa_last_error(), bad
    assert call(D=12) == -2 and b"divisible" in L.cwfa_last_error()          # 12 depths, three levels
    assert call(tab=table(2), D=12) == 0
    assert call(tab=table(3, null_at=1)) == -1 and b"level 1" in L.cwfa_last_error()
    assert call(tab=table(3, bs=31), B=2) == -1 and b"batch stride of level 0" in L.cwfa_last_error()
    assert call(B=2, obs=63) == -1 and b"batch stride of out" in L.cwfa_last_error()
    assert call(tab=table(_lib.NLL_MAX_LEVELS), D=256) == 0 and call(B=3, D=0) == 0 and call(B=3, HW=0) == 0


def test_python_wrappers_refuse_before_any_launch():
    from cwfa_amd import CWFA, ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.chain_nll_map(torch.zeros(1, 4, 4, 8), [])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nll_compose([torch.zeros(1, 4, 4, 8), torch.zeros(1, 2, 4, 8)])
    with pytest.raises(ValueError, match="levels"):
        ops.nll_compose([])
    with pytest.raises(ValueError, match="levels"):
        ops.nll_compose([torch.zeros(1, 1, 1, 1)] * 9)
    # the coverage readout is plain torch: the expected column is the normal's
    obs, exp = CWFA.zscore_coverage([torch.tensor([0.5, -1.5, 2.5, -3.5])], ks=(1.0, 2.0, 3.0))
    assert obs.tolist() == [[0.25, 0.5, 0.75]]
    assert [round(v, 4) for v in exp.tolist()] == [0.6827, 0.9545, 0.9973] and exp[1] == math.erf(2.0 / math.sqrt(2.0))
    with pytest.raises(ValueError):
        CWFA.zscore_coverage([])
