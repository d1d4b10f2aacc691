"""GPU (MI355X): the step schedule of csrc/conv_split3x3.hip -- two weight slots, ONE barrier per step in the middle of the step
(the skip-add forms: at the step boundary), the next step's first A and B fragments requested inside the last n-tile of the step
before -- at the smallest shapes at which it can go wrong (tests/split3x3_midstep_cases.py: the case list and why each size is in it).

Per launch two things are asserted:
  1. against the float64 convolution the bounds of tests/test_gpu_split_dispatch.py: 5e-6 (max-rel and l2-rel) in split precision
     (coupling epilogue: 1e-5, its fast atan / exp), the `check16` rule in one-product mode (2e-5 against float64 of the operands
     rounded as the kernel rounds them, the other 16-bit format's reference at least 10x further away);
  2. the output equals BIT FOR BIT what the parent commit's kernel wrote for the same inputs: a schedule change moves waits,
     barriers and the order between accumulators, never the MFMAs of one accumulator or their order.  The parent's outputs are
     SHA-256 digests in tests/golden/g28_split3x3_parent_bits.json (tools/make_split3x3_bits.py, run with the parent's checkout).
The `out_stats` buffer is summed with float64 atomics and is not bit-stable: it is held to the statistics contract of
test_gpu_split_dispatch.py, and the y written beside it to bit equality with the launch without statistics."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import split3x3_midstep_cases as M
from conftest import assert_close
from split_ref import F16_TOL, _pro32, b16, check16, h, maxrel

pytestmark = pytest.mark.gpu
SPLIT_TOL = 5e-6
COUPLE_TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", M.GOLDEN_NAME)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _restore():
    from cwfa_amd import ops
    keep = ops.SPLIT_3X3_MIN_COUT, ops.SPLIT_3X3_NARROW_MAX
    with torch.no_grad():
        yield
    ops.SPLIT_3X3_MIN_COUT, ops.SPLIT_3X3_NARROW_MAX = keep
    ops.set_option("split3x3_xcd_map", 1)
    ops.set_precision("fp32")


@pytest.fixture(scope="module")
def parent_bits():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["parent_commit"]) == 40
    return g["digests"]


_LIN = {}


def linear(c, aff, add, rnd):
    """float64 convolution (no bias) over the whole bank of the operands rounded by rnd (None: exact); once per key, shared by the
    operand formats"""
    k = (c.name, aff, add, None if rnd is None else rnd.__name__)
    if k not in _LIN:
        t = M.inputs(c)
        r = rnd or (lambda v: v.double())
        xin = _pro32(t["x"], t["sc"] if aff else None, t["sh"] if aff else None, t["add"] if add else None)     # fp32, exact (dyadic grid)
        _LIN[k] = F.conv2d(r(xin), r(t["w"]), padding=t["w"].shape[-1] // 2)
    return _LIN[k]


def reference(c, r, rnd):
    """-> (output, log-det or None) of variant r in float64"""
    t = M.inputs(c)
    if c.form == "couple":
        n, clamp = M.FORMS[c.form][0], 1.7
        lin = linear(c, False, False, rnd) + t["b"].double().view(1, -1, 1, 1)
        s = clamp * 0.636 * torch.atan(lin[:, :n])
        return torch.exp(s) * t["xh"].double() + lin[:, n:], s.sum(dim=(1, 2, 3))
    cout = r["cout"]
    lin = linear(c, r["aff"], r["add"], rnd)[:, :cout] + t["b"][:cout].double().view(1, -1, 1, 1)
    if r["act"] == "prelu":
        lin = torch.where(lin > 0, lin, t["alpha"][:cout].double().view(1, -1, 1, 1) * lin)
    return lin, None


def check_stats(y, st, what):
    """the statistics contract of test_gpu_split_dispatch.py: (sum y, sum y^2) per channel of the kernel's own y"""
    n = y.shape[0] * y.shape[2] * y.shape[3]
    ref64 = torch.stack([y.double().sum((0, 2, 3)), (y.double() ** 2).sum((0, 2, 3))], 1).cpu()
    got = st.cpu().view(-1, 2)
    scale = float(ref64[:, 1].max().sqrt()) * n ** 0.5          # |sum| <= sqrt(n * sumsq)
    assert float((got[:, 0] - ref64[:, 0]).abs().max()) <= 2e-6 * scale, (what, "sum y")
    assert float(((got[:, 1] - ref64[:, 1]) / ref64[:, 1]).abs().max()) <= 2e-6, (what, "sum y^2")


@pytest.mark.parametrize("c,fmt", M.PARAMS, ids=M.PARAM_IDS)
def test_midstep_vs_float64_and_parent_bits(c, fmt, parent_bits):
    from cwfa_amd import ops
    ops.set_precision(fmt)
    res = M.run_case(ops, c, fmt)
    moved = []
    for variant, r in res.items():
        what = f"{c.name} {variant} {fmt}"
        y = r["y"]
        assert y.shape[0] == M.B and y.shape[2:] == (c.H, c.W), what
        if "same_as" in r:
            assert torch.equal(y, res[r["same_as"]]["y"]), (what, "differs from", r["same_as"])
            if "stats" in r:
                check_stats(y, r["stats"], what)
            continue
        if fmt == "split_bf16":
            ref, lref = reference(c, r, None)
            print(f"{what}: max-rel {maxrel(y, ref):.3e}")
            assert_close(y, ref, COUPLE_TOL if c.form == "couple" else SPLIT_TOL, what)
        else:
            own, other = (b16, h) if fmt == "bf16" else (h, b16)
            ref, lref = reference(c, r, own)
            print(f"{what}: max-rel {maxrel(y, ref):.3e}")
            check16(y, ref, reference(c, r, other)[0], what)
        if "logdet" in r:
            e = maxrel(r["logdet"], lref)
            assert e <= (COUPLE_TOL if fmt == "split_bf16" else F16_TOL), (what, "log-det", e)
        if M.digest(y) != parent_bits[M.key(c, fmt, variant)]:
            moved.append(variant)
    assert not moved, (c.name, fmt, "output bits differ from the parent commit's kernel", moved)


def test_parent_bits_cover_the_case_list(parent_bits):
    """one digest per launch that is compared by digest, none left over from another case list"""
    n = {"c256": lambda fmt: 4 if fmt == "fp16" else 8, "couple": lambda fmt: 1, "k7": lambda fmt: 1}
    want = sum(n.get(c.form, lambda fmt: 2)(fmt) for c, fmt in M.PARAMS)
    assert len(parent_bits) == want
    assert all(k.split("/")[0] in ("split_bf16", "bf16", "fp16") and k.split("/")[1] in {c.name for c in M.CASES} for k in parent_bits)
