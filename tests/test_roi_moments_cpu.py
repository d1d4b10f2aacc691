"""CPU: the algebra behind the exact ROI-mean moments of a CAT pyramid -- the restated formula
(tests/roi_moments_ref.py) against the reference fixture g26_roi_moments (tools/make_roi_moments_golden.py: the reference's autograd)
and against the brute-force w1^T J J^T w2 of the dense Jacobian of the restated inverse; the q table against the Haar synthesis of a
box indicator; and the argument validation of cwfa_chain_inv_roi_cov_f32 through the built library (no launch).

Errors of a covariance are relative to the SUM OF THE ABSOLUTE TERMS of that pair (the terms cancel: a whole-depth box sums to zero)."""
import ctypes

import numpy as np
import torch

from conftest import load_golden

import posterior_ref as R
import roi_moments_ref as M
from test_posterior_cpu import _jacobian, _stages, oracle_inverse_stages


def _rel_to_terms(got, want, mag, zero_tol=0.0):
    """max |got - want| / mag over the pairs that have terms; NaN exactly where want is NaN; where there are no terms got is an exact
    zero and want is one too (up to ``zero_tol``, for a want that was formed by differences)."""
    got, want, mag = (np.asarray(a, dtype=np.float64) for a in (got, want, mag))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    live = ~np.isnan(want) & (mag > 0)
    dead = ~np.isnan(want) & (mag == 0)
    assert np.all(got[dead] == 0.0) and np.all(np.abs(want[dead]) <= zero_tol)
    return float((np.abs(got - want)[live] / mag[live]).max())


def fixture_steps(fx, dtype=torch.float64):
    """The fixture's two steps in execution order as (stages, shape): the CPU oracle's coefficients (test_posterior_cpu)."""
    steps = []
    for ix in (1, 0):
        sub = {k[len(f"s{ix}/"):]: v for k, v in fx.items() if k.startswith(f"s{ix}/")}
        steps.append((oracle_inverse_stages(sub, dtype), tuple(sub["c0"].shape)))
    return steps


def test_restatement_vs_fixture():
    fx = load_golden("g26_roi_moments")
    steps = fixture_steps(fx)
    assert [s[1] for s in steps] == [(2, 2, 12, 16), (2, 4, 12, 16)]
    var, var_mag = M.roi_cov(steps, 1.0, fx["boxes"])
    cov, cov_mag = M.roi_cov(steps, 1.0, fx["boxes"], fx["pairs"])
    e_var = _rel_to_terms(var, fx["var_unit"], var_mag)
    e_cov = _rel_to_terms(cov, fx["cov_unit"], cov_mag)
    print(f"[roi moments] restatement vs fixture: var {e_var:.3e}, cov {e_cov:.3e}")
    assert e_var <= 1e-12 and e_cov <= 1e-12
    # the fixture's own sums of absolute terms are the restatement's
    assert _rel_to_terms(var_mag, fx["abs_unit_var"], var_mag) <= 1e-12
    assert _rel_to_terms(cov_mag, fx["abs_unit_cov"], cov_mag) <= 1e-12
    # what the fixture is for
    assert np.all(fx["cov_unit"][:, 0] > 0) and np.all(fx["cov_unit"][:, 1] < 0) and np.all(fx["cov_unit"][:, 2] == 0)
    assert np.all(var[:, 2] <= 1e-24 * np.nanmax(var)) and np.all(np.isnan(var[:, 4]))
    assert np.abs(fx["var_unit"][:, 0] / fx["voxel_factor"] - 1.0).max() <= 1e-12
    # and the mean: the ROI means of the restated z = 0 volume
    up = torch.from_numpy(fx["low"]).double()
    for stages, _ in steps:
        up = R.chain_inv(None, up, stages)
    for r, (z0, z1, y0, y1, x0, x1) in enumerate(fx["boxes"]):
        if (z1 - z0) * (y1 - y0) * (x1 - x0):
            got = up[:, z0:z1, y0:y1, x0:x1].mean(dim=(1, 2, 3)).numpy()
            assert np.abs(got - fx["roi_mean0"][:, r]).max() <= 1e-12 * np.nanmax(np.abs(fx["roi_mean0"]))


def test_restatement_vs_bruteforce_jacobian():
    """Two stacked hand-built steps, C0 = 2, H = 3, W = 5 (D = 8): six stages each with gathers on all three axes, an s-less and a
    t-less stage, all four clamp kinds.  Cov = z_var * w1^T J J^T w2 with w_r = indicator / cnt over the dense Jacobian."""
    g = torch.Generator().manual_seed(19)
    sa, sb = (1, 2, 3, 5), (1, 4, 3, 5)
    kinds = ["ATAN", "TANH", "NONE", "SIGMOID", "NONE", "ATAN"]
    st_a = _stages(sa, g, [None, 3, 2, 3, 1, 2], no_s=(3,), no_t=(1,), kinds=kinds)
    st_b = _stages(sb, g, [3, 1, None, 2, 3, 1], no_s=(2,), no_t=(4,), kinds=kinds[::-1])
    st_b[4]["clamp"] = 0.5
    low = torch.randn(sa, generator=g, dtype=torch.float64)
    na, nb = 30, 60

    def pyramid(zz):
        return R.chain_inv(zz[na:].view(sb), R.chain_inv(zz[:na].view(sa), low, st_a), st_b)

    J = _jacobian(pyramid, na + nb).numpy()                  # [8 * 15, 90]
    D, H, W = 8, 3, 5
    boxes, pairs = M.box_catalogue(D, H, W)
    z_var = 0.29112509477279314

    def weight(b):
        w = np.zeros((D, H, W))
        n = (b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4])
        if n == 0:
            return None
        w[b[0]:b[1], b[2]:b[3], b[4]:b[5]] = 1.0 / n
        return w.ravel() @ J

    all_pairs = np.concatenate([np.repeat(np.arange(len(boxes))[:, None], 2, 1), pairs])
    want = np.zeros((1, len(all_pairs)))
    for p, (r1, r2) in enumerate(all_pairs):
        w1, w2 = weight(boxes[r1]), weight(boxes[r2])
        want[0, p] = np.nan if w1 is None or w2 is None else z_var * float(w1 @ w2)
    got, mag = M.roi_cov([(st_a, sa), (st_b, sb)], z_var, boxes, all_pairs)
    err = _rel_to_terms(got, want, mag, zero_tol=1e-15 * np.nanmax(np.abs(want)))     # the Jacobian's columns are differences
    print(f"[roi moments] restatement vs brute force: {err:.3e}")
    assert err <= 1e-12
    R_ = len(boxes)
    assert want[0, R_ + 0] > 0 and want[0, R_ + 1] < 0 and got[0, R_ + 2] == 0 and got[0, 2] == 0
    # pairs = None is the diagonal
    diag, _ = M.roi_cov([(st_a, sa), (st_b, sb)], z_var, boxes)
    assert np.array_equal(diag, got[:, :R_], equal_nan=True)


def test_q_table_is_the_haar_analysis_of_the_indicator():
    """D = 16, m = 1 .. 4, every [z0, z1): the weight of v_m[c] summed over the box is q_m(c) * 2^(-m/2), blocks wholly inside or outside
    give 0, and the details with those weights plus the mean of the indicator synthesise the indicator again."""
    D, L = 16, 4
    Ws = M.haar_synthesis_weights(D, L)
    for z0 in range(D + 1):
        for z1 in range(z0, D + 1):
            ind = np.zeros(D)
            ind[z0:z1] = 1.0
            synth = np.full(D, (z1 - z0) / D)
            for m in range(1, L + 1):
                q = M.q_table(z0, z1, m, D >> m)
                coeff = Ws[m - 1].T @ ind
                assert np.abs(coeff - q * 2.0 ** (-m / 2)).max() <= 1e-15
                for c in range(D >> m):
                    lo, hi = c << m, (c + 1) << m
                    if (z0 <= lo and hi <= z1) or hi <= z0 or z1 <= lo:
                        assert q[c] == 0
                assert np.count_nonzero(q) <= 2               # only the blocks that hold an end of the range
                synth = synth + Ws[m - 1] @ (q * 2.0 ** (-m / 2))
            assert np.abs(synth - ind).max() <= 1e-14


def test_entry_point_validation():
    """The argument checks of cwfa_chain_inv_roi_cov_f32 (codes of include/cwfa_hip.h): every rejected call returns before a launch."""
    from cwfa_amd import _lib, build
    build.build_all()
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ch = _lib.Chain()
    ch.n_stages = 1
    ch.stage[0].s_raw = p.value
    ch.stage[0].s_bs = 4 * 8 * 8
    ch.stage[0].clamp_kind = 1
    ch.stage[0].clamp = 2.0
    ch.stage[0].pre_scale = 1.0
    ch.stage[0].perm_axis = 1
    box = lambda *v: (ctypes.c_int32 * len(v))(*v)            # noqa: E731
    ok = box(0, 3, 0, 8, 0, 8)

    def call(out=p, chain=ch, z_var=1.0, B=1, C=4, H=8, W=8, level=1, boxes=ok, R=1, pairs=None, P=1, out_bs=1):
        return L.cwfa_chain_inv_roi_cov_f32(out, ctypes.byref(chain), z_var, B, C, H, W, level, boxes, R, pairs, P, None, out_bs, None)

    E_INVAL, E_SHAPE = -1, -2
    assert call(out=None) == E_INVAL and b"null" in L.cwfa_last_error()
    for bad in ([0, 9, 0, 8, 0, 8], [0, 3, 0, 9, 0, 8], [0, 3, 0, 8, -1, 8], [3, 2, 0, 8, 0, 8]):    # D = 4 * 2 = 8
        assert call(boxes=box(*bad)) == E_INVAL and b"not inside" in L.cwfa_last_error()
    assert call(level=2, boxes=box(0, 16, 0, 8, 0, 8), B=0) == 0               # the same box is inside at level 2
    assert call(pairs=box(0, 1), P=1) == E_INVAL and b"outside [0, 1)" in L.cwfa_last_error()
    assert call(pairs=box(-1, 0), P=1) == E_INVAL
    assert call(P=2) == E_INVAL and b"without a pair table" in L.cwfa_last_error()
    for m in (0, -1, 31):
        assert call(level=m) == E_INVAL and b"level" in L.cwfa_last_error()
    gin = _lib.Chain.from_buffer_copy(ch)
    gin.stage[0].gin = 1
    assert call(chain=gin) == E_INVAL and b"GIN" in L.cwfa_last_error()
    for zv in (-0.5, float("nan"), float("inf")):
        assert call(z_var=zv) == E_INVAL and b"z_var" in L.cwfa_last_error()
    assert call(B=-1) == E_SHAPE
    assert call(out_bs=0) == E_INVAL and b"stride" in L.cwfa_last_error()
    assert call(C=1 << 20, level=30) == E_SHAPE
    # empty problems are accepted and launch nothing
    assert call(B=0) == 0
    assert call(boxes=None, R=0, P=0, out_bs=0) == 0
