"""CPU: the exact data set and the restated host selection of tests/layer_ref.py checked on their own, and the case lists of
tests/test_gpu_layer_dispatch.py (imported as data) checked to reach all 13 forms of the fused split layer in each operand format."""
import pytest
import torch
import torch.nn.functional as F

import layer_ref as R
import test_gpu_layer_dispatch as G

SMALL_SETS = sorted({(c.shape, c.cin) for c in G.SMALL})


def test_case_lists_reach_every_form_in_every_format():
    assert len(R.ALL_FORMS) == 13 and len(R.FORMATS) == 3
    for cases in ([(c.form, c.cin + 1) for c in G.SMALL], [(f, 13) for f in G.WALK_FORMS]):
        assert {(fmt, f.key(u_ch)) for fmt in R.FORMATS for f, u_ch in cases} == {(fmt, k) for fmt in R.FORMATS for k in R.ALL_FORMS}
    # what the issue of the case list asks: every form at the first four shapes, every u_ch at (2,17,45), the NCHW forms misaligned
    for f in G.FORMS:
        assert {c.shape for c in G.SMALL if c.form == f} >= set(G.SHAPES[:4])
        assert (f.layout == 0) == any(c.mis for c in G.SMALL if c.form == f)
    assert {c.cin + 1 for c in G.SMALL if c.shape == (2, 17, 45) and c.form.entry == "first"} == {13, 16, 17, 32}
    assert {c.cin + 1 for c in G.SMALL if c.form.short} == {13, 16}
    assert G.RANDOM_CIN + 1 <= 16                               # the random-data chains include the short form


def test_select_restates_the_host_rules():
    S = R.select
    assert S("plain", 3) == (2, False, False, False, True, True) and S("plain", 1) == (2, False, False, False, True, False)
    assert S("tape", 0, hid=True) == (2, True, False, False, False, False)
    assert S("tape", 1, hid=True) is None and S("tape", 0) is None                    # tape: NCHW only, and a hidden map
    assert S("first", 3, u_ch=13) == (1, False, False, False, True, True)
    # x = NULL: layout &= 2 -- the input bit means nothing
    assert S("first", 1, x_none=True, u_ch=13) == S("first", 0, x_none=True, u_ch=13) == (1, False, True, False, False, False)
    assert S("first", 3, x_none=True, u_ch=13) == S("first", 2, x_none=True, u_ch=13) == (1, False, True, False, False, True)
    assert S("first", 2, x_none=True, short=True, u_ch=16) == (1, False, True, True, False, True)
    assert S("first", 0, x_none=True, short=True, u_ch=17) is None and S("first", 0, short=True, u_ch=13) is None
    assert S("first", 0, u_ch=0) is None and S("first", 0, u_ch=33) is None and S("plain", 4) is None and S("plain", -1) is None
    reach = {S(e, l, x_none=xn, short=sh, hid=hd, u_ch=13) for e in ("plain", "tape", "first") for l in range(4)
             for xn in (False, True) for sh in (False, True) for hd in (False, True)}
    assert reach - {None} == R.ALL_FORMS


@pytest.mark.parametrize("shape,cin", SMALL_SETS, ids=[f"{'x'.join(map(str, s))}-c{c}" for s, c in SMALL_SETS])
def test_exact_data_premises(shape, cin):
    """the premises at every shape and cin of the GPU file (exact_layer_data asserts them); and the recipe's own claims restated: the
    first-layer forms compute the same integers from u, and float64 rounded to fp32 is the idealised integer result"""
    d = R.exact_layer_data(shape[0], cin, *shape[1:], seed=1)
    wt, r, x, u = d["wt"], d["ref"], d["x"], d["u"]
    assert set(u.unique().tolist()) <= {-1.0, 0.0, 1.0} and float(x.abs().max()) <= 3
    assert torch.equal(x, F.conv2d(u, wt["w0"], wt["b0"]))
    assert bool(((wt["w0"] != 0).sum((1, 2, 3)) == 2).all()) and bool(((wt["w3"] != 0).sum((1, 2, 3)) == 24).all())
    assert bool(((wt["w1"] != 0).sum((1, 2, 3)) == 8).all())
    # the idealised layer in integer arithmetic: ELU = identity at >= 0, -1 at <= -20
    xi = x.to(torch.int64)
    pre3 = F.conv2d(x.double(), wt["w3"].double(), padding=1).round().to(torch.int64) + wt["b3"].to(torch.int64).view(1, 64, 1, 1)
    hid = torch.where(pre3 >= 0, pre3, torch.full_like(pre3, -1))
    pre1 = torch.einsum("om,bmhw->bohw", wt["w1"].view(64, 64).to(torch.int64), hid) + wt["b1"].to(torch.int64).view(1, 64, 1, 1) + xi
    y = torch.where(pre1 >= 0, pre1, torch.full_like(pre1, -1))
    assert torch.equal(r["hidden"].float(), hid.float()) and torch.equal(r["y"].float(), y.float())
    assert int(y.max()) < 2 ** 24 and int(hid.max()) <= R.HID_MAX
    # the composed first layer: conv3x3'(u | 1) + W0' (u | 1) gives the same integers (zero padding included)
    w3c, w0c = R.compose_first_layer(wt["w0"], wt["b0"], wt["w3"])
    u1 = torch.cat([u, torch.ones(shape[0], 1, *shape[1:])], 1).double()
    assert torch.equal(F.conv2d(u1, w3c[:, :cin + 1].double(), wt["b3"].double(), padding=1), r["pre3"])
    assert torch.equal(F.conv2d(u1, w0c[:, :cin + 1].double().view(64, cin + 1, 1, 1)), x.double())
    assert not bool(w3c[:, cin + 1:].any()) and not bool(w0c[:, cin + 1:].any())


def test_premises_notice_an_inexact_recipe():
    d = R.exact_layer_data(1, 12, 16, 32, seed=1)
    bad = {**d, "ref": {**d["ref"], "pre1": d["ref"]["pre1"] - (R.S1 + 5)}}        # a pre-activation inside (-20, 0)
    with pytest.raises(AssertionError):
        R.check_premises(bad)
    bad = {**d, "x": d["x"] + 1.0 / 512}                                            # a value bf16 does not hold
    with pytest.raises(AssertionError):
        R.check_premises(bad)
    bad = {**d, "ref": {**d["ref"], "hidden": d["ref"]["hidden"] + 200}}
    with pytest.raises(AssertionError):
        R.check_premises(bad)


def test_blocked_round_trip():
    t = torch.arange(2 * 64 * 3 * 5, dtype=torch.float32).view(2, 64, 3, 5)
    b = R._to_blocked(t)
    assert torch.equal(R._from_blocked(b), t)
    assert float(b.view(2, 8, 3, 5, 8)[1, 2, 1, 4, 3]) == float(t[1, 2 * 8 + 3, 1, 4])


def test_walk_geometry():
    """the MI355X (256 CUs): the geometries the issue of the walk names, and their premises"""
    for second in (False, True):
        B, H, W, T, total = R.walk_premises(256, second)
        assert total // 256 >= 3 and total - 3 * 256 >= 8
    assert R.walk_geometry(256) == (4, 123, 791, 200, 800) and R.walk_geometry(256, True) == (4, 107, 919, 203, 812)
    with pytest.raises(AssertionError):
        R.walk_premises(100)                                    # (a CU count that is no multiple of 8: the tile map would be off)
