"""CPU: the algebra behind the posterior of a CAT pyramid -- the variance of the truncated latent, the
variance recursion against the brute-force Jacobian of the restated inverse chain, and the reference fixture g24_posterior
(tools/make_posterior_golden.py) against the recursion fed by the CPU oracle's coefficients."""
import numpy as np
import pytest
import torch

from conftest import assert_close, load_golden, sd_of

import posterior_ref as R


# ------------------------------------------------------------------------------------------------ z_var(T)
def test_truncated_normal_variance_known_values():
    from cwfa_amd.CWFA import truncated_normal_variance as zv
    assert zv(0) == 0.0 and zv(0.0) == 0.0
    assert abs(zv(1) - 0.29112509477279314) <= 1e-15
    assert zv(float("inf")) == 1.0
    assert abs(zv(40.0) - 1.0) <= 1e-15
    for T in (1e-6, 1e-5, 1e-4, 1e-3):                       # -> T^2/3 (next term: -2 T^4 / 45)
        assert abs(zv(T) / (T * T / 3.0) - 1.0) <= 0.2 * T * T + 1e-15, T


def test_truncated_normal_variance_is_non_decreasing():
    from cwfa_amd.CWFA import truncated_normal_variance as zv
    grid = np.concatenate([np.logspace(-8, 0, 400), np.linspace(0.3, 0.7, 801), np.linspace(1.0, 12.0, 600)])   # dense around the series / closed-form switch
    grid.sort()
    vals = [zv(float(T)) for T in grid]
    assert all(b >= a for a, b in zip(vals, vals[1:]))
    assert 0.0 < vals[0] and vals[-1] <= 1.0


@pytest.mark.parametrize("T", [1e-6, 1e-3, 0.1, 0.7, 1, 3, 10])
def test_truncated_normal_variance_vs_quadrature(T):
    from cwfa_amd.CWFA import truncated_normal_variance as zv
    want = R.z_var(T)
    assert abs(zv(T) - want) <= 1e-9 * want, (T, zv(T), want)


def test_truncated_normal_variance_rejects_negative():
    from cwfa_amd.CWFA import truncated_normal_variance as zv
    with pytest.raises(ValueError):
        zv(-1)
    with pytest.raises(ValueError):
        zv(float("nan"))


# ------------------------------------------------------------------------------------------------ recursion vs brute force
def _stages(shape, g, axes, no_s=(), no_t=(), kinds=None):
    B, C, H, W = shape
    out = []
    for k, ax in enumerate(axes):
        st = {"s_raw": None if k in no_s else torch.randn(shape, generator=g, dtype=torch.float64),
              "t": None if k in no_t else torch.randn(shape, generator=g, dtype=torch.float64),
              "perm": None if ax is None else torch.randperm([0, C, H, W][ax], generator=g), "axis": ax,
              "kind": (kinds or ["ATAN"] * len(axes))[k], "clamp": 2.0, "pre": 1.0, "neg": k == 0}
        out.append(st)
    return out


def _jacobian(fn, n_in):
    """Columns fn(e_j) - fn(0) of an affine map, as [n_out, n_in]."""
    base = fn(torch.zeros(n_in, dtype=torch.float64))
    cols = []
    for j in range(n_in):
        e = torch.zeros(n_in, dtype=torch.float64)
        e[j] = 1.0
        cols.append((fn(e) - base).reshape(-1))
    return torch.stack(cols, 1)


def test_variance_recursion_vs_bruteforce_jacobian():
    """(1, 2, 3, 4), six stages: gathers on axes 1, 2, 3 (two of them column gathers), one s-less and one t-less stage, all four
    clamp kinds.  z_var * diag(J J^T) of the basis-vector Jacobian of the restated inverse to 1e-12 relative."""
    shape = (1, 2, 3, 4)
    g = torch.Generator().manual_seed(11)
    stages = _stages(shape, g, [3, 1, None, 2, 3, 1], no_s=(2,), no_t=(4,), kinds=["ATAN", "TANH", "NONE", "SIGMOID", "NONE", "ATAN"])
    stages[4]["clamp"] = 0.5
    low = torch.randn(shape, generator=g, dtype=torch.float64)
    n = low.numel()
    J = _jacobian(lambda z: R.chain_inv(z.view(shape), low, stages), n)
    z_var = 0.29112509477279314
    want = z_var * (J * J).sum(1).view(1, 4, 3, 4)
    got = R.chain_inv_var(None, stages, z_var, shape)
    assert R.per_element_rel(got, want) <= 1e-12
    # each row of J has exactly one entry: the map is elementwise
    assert int((J != 0).sum()) == J.shape[0]
    # and the equivalent statement the fixture uses: z_var * (x(z = 1) - x(z = 0))^2
    alt = z_var * (R.chain_inv(torch.ones(shape, dtype=torch.float64), low, stages) - R.chain_inv(None, low, stages)) ** 2
    assert R.per_element_rel(got, alt) <= 1e-12
    # the shifts never enter
    for st in stages:
        st["t"] = None
    assert torch.equal(R.chain_inv_var(None, stages, z_var, shape), got)


def test_variance_recursion_two_stacked_steps():
    """Two steps: the coarser one (half the channels) feeds the finer one's low band and var_low; both latents independent."""
    g = torch.Generator().manual_seed(12)
    sa, sb = (1, 1, 3, 4), (1, 2, 3, 4)
    st_a = _stages(sa, g, [None, 3, 2, 3, 1, 2], no_s=(3,), no_t=(1,))
    st_b = _stages(sb, g, [3, 1, None, 2, 3, 1], no_s=(2,), no_t=(4,))
    low = torch.randn(sa, generator=g, dtype=torch.float64)
    na, nb = 12, 24

    def pyramid(zz):
        mid = R.chain_inv(zz[:na].view(sa), low, st_a)
        return R.chain_inv(zz[na:].view(sb), mid, st_b)

    J = _jacobian(pyramid, na + nb)
    z_var = 0.7
    want = z_var * (J * J).sum(1).view(1, 4, 3, 4)
    var_a = R.chain_inv_var(None, st_a, z_var, sa)
    got = R.chain_inv_var(var_a, st_b, z_var)
    assert R.per_element_rel(got, want) <= 1e-12
    assert int((J != 0).sum()) == 2 * J.shape[0]              # one latent of each step per voxel


# ------------------------------------------------------------------------------------------------ the reference fixture
def oracle_inverse_stages(fx, dtype=torch.float32):
    """The inverse direction's stages of the fixture's step from the CPU oracle's own sub-network and clamp (oracle.cwfa_oracle):
    posterior_ref stage dicts with the clamped ``s`` and ``t``."""
    from oracle import cwfa_oracle as O
    sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd_of(fx).items()}
    om, mean = torch.from_numpy(fx["c0"]).to(dtype), torch.from_numpy(fx["c1"]).to(dtype)
    axes = {int(k.split("_")[-1]): int(v) for k, v in fx.items() if k.startswith("meta/axis_")}
    C = om.shape[1]
    stages, pending = [], None
    for kind, i in reversed(O.step_layout("CAT")[2:]):
        p = f"module_list.{i}."
        if kind == "perm":
            if pending is not None:
                stages.append({"perm": pending[0], "axis": pending[1]})
            pending = (sd[p + "perm_inv"], axes.get(i, 1))
            continue
        first = kind == "cat_first"
        a = O.subnet(sd, p + "subnet.", torch.cat((mean, om), 1) if first else om, first)
        st = {"s": O.soft_clamp(a[:, :C], "ATAN", 2.0), "t": a[:, C:]}
        if pending is not None:
            st["perm"], st["axis"] = pending
            pending = None
        stages.append(st)
    if pending is not None:
        stages.append({"perm": pending[0], "axis": pending[1]})
    return stages


def test_fixture_conditions():
    fx = load_golden("g24_posterior")
    vf = fx["var_factor"]
    assert vf.shape == (2, 6, 24, 64) and vf.dtype == np.float64
    assert float(fx["var_factor_min"]) == vf.min() and float(fx["var_factor_max"]) == vf.max()
    assert vf.max() / vf.min() > 100.0                        # more than two decades: a max-normalised measure would hide most of it
    assert np.abs(vf[:, 0::2] / vf[:, 1::2] - 1.0).max() < 1e-10


def test_fixture_vs_oracle_step():
    """The float32 oracle step's coefficients through the restated recursion reproduce the reference's var_factor (and the restated
    chain its x0) within the bound tests/test_oracle_golden.py holds the float32 oracle's flow step to (1e-5, max-normalised
    and L2)."""
    from oracle import cwfa_oracle as O
    fx = load_golden("g24_posterior")
    stages = oracle_inverse_stages(fx)
    low = torch.from_numpy(fx["low"])
    assert_close(R.chain_inv_var(None, stages, 1.0, tuple(low.shape)), fx["var_factor"], 1e-5, "var_factor")
    assert_close(R.chain_inv(None, low, stages), fx["x0"], 1e-5, "x0")
    # the oracle's own flow step agrees with the restated chain fed by its coefficients
    sd = sd_of(fx)
    axes = {int(k.split("_")[-1]): int(v) for k, v in fx.items() if k.startswith("meta/axis_")}
    for i, _ in [(i, k) for k, i in O.step_layout("CAT") if k == "perm"]:
        axes.setdefault(i, 1)
    x0, _ = O.flow_step(sd, (torch.zeros_like(low), low), [torch.from_numpy(fx["c0"]), torch.from_numpy(fx["c1"])], True, axes, "CAT")
    assert_close(x0, fx["x0"], 1e-5, "oracle x0")
    # in float64 the same restatement is the reference's map to rounding (the fixture's own cancellation error is ~1e-12)
    stages64 = oracle_inverse_stages(fx, torch.float64)
    assert R.per_element_rel(R.chain_inv_var(None, stages64, 1.0, tuple(low.shape)), fx["var_factor"]) <= 1e-9
