"""GPU (MI355X): every launch form of the fused coupling chain (cwfa_chain_fwd_f32, cwfa_chain_inv_f32) and the single-stage entry
points cwfa_affine_f32 / cwfa_channel_affine_f32 against the float64 restatements of tests/chain_ref.py on the same fp32 inputs.

Each chain entry picks among three kernels: the 16-byte form chain_rows4_kernel<INV, 6 | CWFA_CHAIN_MAX> (W in {64 .. 1024} with W/4
dividing 256 and every pointer and batch stride on a 16-byte boundary; with or without the LDS exchange of a column gather, with the
caller's composed tables or the dependent walk), the row-staged form (W >= 64, (2 n + 1) W floats <= 60 KiB of LDS) and the general
pull form.  `dispatch` restates that selection; the case list is asserted (at import) to reach every (form, NS, column gather,
tables) tuple in both directions, so a form added later fails the import until it has a case.

Every case runs with x / z / low and every stage's s_raw / t as channel slices of larger tensors whose other channels hold NaN,
writes its outputs into channel slices of NaN-filled tensors (through the library entry point itself: nothing outside the slices
may change, no NaN may appear inside), accumulates log-det and sumsq onto non-zero values, and is repeated without log-det, with the
tables (bit-equal), one sample at a time (bit-equal), through ops.chain_fwd / ops.chain_inv (bit-equal where the form is the same)
and, inverse, with z = None.

The value bound.  The measure is e = max_p |got - ref|[p] / M[p] with M from chain_ref.chain_magnitude, the walk of the chain on
absolute values: v' = exp(s) v + t cancels, so an element's error is relative to exp(s) |v| + |t|, not to |v'|.  With U = 2^-24 (the
relative error of one fp32 rounding) a stage v' = fl(fl(E v) + T), E = exp(s (1 + ..)), adds relative to M'
    clamp * a_kind            the absolute error of s, which is the relative error of exp(s): csrc/common.h states 1.9e-7 for
                              cwfa_atan (times the 0.636 of the clamp) and 2.5e-7 for cwfa_tanh; NONE is fl(clamp * fl(s_raw * pre)),
                              two roundings of |a| <= A: a_kind = 2 A U; SIGMOID is clamp * 2 (1 / (1 + expf(-a)) - 0.5): the argument
                              rounding (A U, slope 1/4), expf (2 U relative, slope 1/4), the sum and the quotient (U each on a value
                              <= 1), the difference (U / 2; exact above 1/4) doubled, and the outer product (U): a_kind = (7 + A / 2) U.
                              (A = 4 pre: the raw coefficients of the cases are clipped to [-4, 4].)
    (S log2(e) + 4) U         S = 2 >= |s|: the fast exponential of the 16-byte form rounds s log2(e) to fp32 before v_exp_f32 (the
                              other forms call expf and do not have this term); 4 U for the exponential itself, the scaling of t and
                              the two roundings of the stage.
A stage without s is fl(v + T) with one rounding in T: 2 U; a stage that only gathers is exact.  The Haar pair adds two roundings,
2 U.  The errors of earlier stages are carried along by the same factors as M, so the budgets add: bound = sum over the stages + 2 U,
2 U for the empty chain and at most 5.4e-6 for the eight ATAN stages of r4_64_8st: below 1e-5 for every case (asserted at import).
The fp32 parameters (pre_scale = fl(0.1)) enter the reference as the kernel receives them.  A dropped gather, a wrong t convention
or a wrong sign of s sit at 0.1 to 2 on this measure.
Single stage (cwfa_affine_f32): the stage budget alone, with expf; the GIN stage adds (C + 3) S U for the fp32 channel mean of C
terms and its subtraction.  cwfa_channel_affine_f32: two roundings, 2 U relative to |x scale| + |shift| (mode 1: to that over |scale|).

low (forward): within one ulp of the fp32 (e + o) * fl(1 / sqrt 2), identical between the forms.  log-det: |got - (initial +- sum
of s)| <= 8 U * sum |s| per sample.  sumsq: the float64 sum of squares of the kernel's own z to 1e-12.

The empty chain's 2 U leaves no room for the 1.7e-8 by which fl(1 / sqrt 2) is off; its two exactly rounded operations give the same
figure on every machine (1.18e-7 on the seeded data), which is below 2 U.

Largest e measured on an MI355X (every test prints its figure next to the bound, pytest -s; plain fp32 torch on the CPU gives
7.0e-7 / 4.4e-7 / 5.1e-7 on the same cases: `python tests/test_gpu_chain_dispatch.py`):
  16-byte form   forward 7.4e-7 (r4_1024_8col; bound 5.3e-6), inverse 7.3e-7 (r4_64_8st; 5.3e-6); the empty chain 1.18e-7 of 1.19e-7
  row-staged     forward 5.0e-7, inverse 4.8e-7 (rows_mis_zx; 3.5e-6)
  general        forward 5.0e-7, inverse 6.1e-7 (gen_wide; 4.0e-6)
  round trip     3.8e-7 (r4_1024_8col; 1.07e-5); row-staged against 16-byte form 3.8e-7 (6.9e-6)
  log-det        at most 0.14 of its bound (gen_small_1, three positions), 0.007 of it in the round trips
  one stage      plain 3.3e-7 (1.04e-6), GIN 2.6e-7 (1.08e-6); channel affine 1.15e-7 (1.19e-7; exactly rounded), there and back 1.7e-7 (2.4e-7)
Every case passed with the kernels as they stand: no kernel was changed.  With chain_rows4_kernel edited in place (never committed) the
file fails as it should: without the `else ssum = 0.f` of the dead rows the log-det of r4_64_dead, r4_128_nocol, r4_256_nocol_7st and
r4_512; with one exchange buffer (`nx & 0`) the values of r4_1024_8col, r4_512_6col and r4_1024 (rows of one wave, W <= 256, cannot
show it); with t_neg_div_sqrt2 ignored or the sign of s swapped in __expf every case of the 16-byte form that has a stage."""
import ctypes as C
import math
import zlib
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import chain_ref as R
from test_gpu_conv_dispatch import NAN, NAN_BITS, nan_around, untouched_outside

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
S_MAX = 2.0                                   # |s| <= 2 in every stage of every case (asserted on the references)
RAW_MAX = 4.0                                 # the raw coefficients are clipped to [-RAW_MAX, RAW_MAX]
LOG2E = math.log2(math.e)
ATAN_ERR, TANH_ERR = 1.9e-7, 2.5e-7           # csrc/common.h: cwfa_atan, cwfa_tanh
PRE01 = float(np.float32(0.1))                # pre_scale = 0.1 as the kernel receives it
LDS_CAP = 60 * 1024
CHAIN_THREADS = 256

# the stage mix, cycled (and rotated per case): kind, clamp, pre_scale; the stage at slot 4 has no s, the one at slot 1 no t
MIX = {"atan": [("ATAN", 2.0, 1.0)] * 8,
       "mixed": [("NONE", 0.5, 1.0), ("ATAN", 2.0, 1.0), ("TANH", 2.0, PRE01), ("SIGMOID", 1.5, 1.0), ("ATAN", 2.0, 1.0), ("TANH", 1.0, 1.0),
                 ("SIGMOID", 2.0, PRE01), ("NONE", 0.5, 1.0)]}
NO_S_SLOT, NO_T_SLOT = 4, 1
MIS_K = 2                                     # the stage whose s_raw / t the misaligned cases shift


@dataclass(frozen=True)
class Case:
    name: str
    shape: tuple              # (B, C, H, W) of z / low; x has 2 C channels
    axes: tuple               # per stage: the gather's axis (1 / 2 / 3) or None
    mix: str = "atan"
    rot: int = 0              # rotation of the mix
    final: bool = False       # forward: a final channel permutation
    tables: bool = False      # launched with ops.chain_tables (and compared bitwise with the walk)
    mis: str = ""             # one operand one float past a 16-byte boundary: "zx" (z inverse / x forward), "low", "s", "t", "out" (x / z);
                              # "bs": aligned pointers, but a batch stride of z / x that is no multiple of four floats
    data: str = ""            # take the data of the case of this name

    def slot(self, k):
        return (k + self.rot) % 8

    def has_s(self, k):
        return self.mix == "atan" or self.slot(k) != NO_S_SLOT

    def has_t(self, k):
        return self.mix == "atan" or self.slot(k) != NO_T_SLOT

    def param(self, k):
        return MIX[self.mix][self.slot(k)]


# ------------------------------------------------------------------------------------------------ the host selection, restated
def rows4_shape(W):
    return W >= 64 and W % 4 == 0 and W // 4 <= CHAIN_THREADS and CHAIN_THREADS % (W // 4) == 0


def dispatch(c, inv=False, z_none=False):
    """(form, NS, column gather, tables) that case c reaches in cwfa_chain_fwd_f32 (inv: cwfa_chain_inv_f32): chain_rows4_ok, then
    chain_rows_ok, then the general kernel.  A z that is not passed cannot be misaligned."""
    W, n = c.shape[3], len(c.axes)
    mis = c.mis and not (c.mis in ("zx", "bs") and inv and z_none)
    if rows4_shape(W) and not mis:
        return ("rows4", 6 if n <= 6 else 8, 3 in c.axes, c.tables)
    if W >= 64 and (2 * n + 1) * W * 4 <= LDS_CAP:
        return ("rows", None, None, None)
    return ("general", None, None, None)


TUPLES = ({("rows4", ns, col, tab) for ns in (6, 8) for col in (False, True) for tab in (False, True)}
          | {("rows", None, None, None), ("general", None, None, None)})


def _both(name, shape, axes, **kw):
    return [Case(name, shape, tuple(axes), **kw), Case(name + "_tab", shape, tuple(axes), tables=True, data=name, **kw)]


DEAD_AXES = (None, 3, 1, 2, 3, 1)
CASES = [
    # ---- 16-byte form
    *_both("r4_64_dead", (2, 3, 24, 64), DEAD_AXES, mix="mixed", final=True),         # 16 rows per block, the second block half dead, both buffers
    *_both("r4_64_8st", (2, 3, 16, 64), (3, 1, 3, 2, 3, None, 3, 1)),                   # NS = 8; four column gathers: buffer 0 reused twice
    *_both("r4_128_nocol", (2, 2, 9, 128), (1, 2, None, 1, 2, 1), mix="mixed", rot=3, final=True),      # lds = 0, RB = 8 with dead rows
    *_both("r4_256_nocol_7st", (2, 2, 5, 256), (1, 2, None, 2, 1, 2, 1)),               # NS = 8 without the exchange, RB = 4 with dead rows
    *_both("r4_512", (1, 2, 3, 512), (None, 3, 2, 1, 3, 2)),                            # RB = 2, a dead row
    *_both("r4_1024", (1, 2, 3, 1024), (3, 1, 2, 3, None, 1), mix="mixed", rot=1, final=True),          # one row per block, tpr = 256
    # rows of more than one wave (W > 256), a column gather in every stage, 32 blocks: if the exchange were not double-buffered, a fast
    # wave would overwrite values a slow one still has to read -- wave-local rows (W <= 256) cannot show that
    Case("r4_1024_8col", (2, 2, 8, 1024), (3,) * 8),
    Case("r4_512_6col", (2, 2, 8, 512), (3,) * 6, mix="mixed", final=True),
    *_both("r4_1stage", (2, 2, 16, 64), (3,), mix="mixed", rot=2, final=True),
    *_both("r4_0stage", (2, 2, 16, 64), ()),                                            # the Haar split / merge alone
    # ---- row-staged form
    *_both("rows_96", (2, 3, 5, 96), (3, 1, None, 2, 3, 1), mix="mixed", final=True),   # W / 4 = 24 does not divide 256
    Case("rows_300", (1, 2, 3, 300), (None, 3, 1, 2, 3), mix="mixed", rot=5),           # the w += 256 wrap
    # ---- the r4_64_dead chain with one operand off the 16-byte grid (or, "bs", its second sample only): each clause of chain_rows4_ok's
    # alignment test
    *[Case("rows_mis_" + m, (2, 3, 24, 64), DEAD_AXES, mix="mixed", final=True, mis=m, data="r4_64_dead") for m in ("zx", "low", "s", "t", "out", "bs")],
    # ---- general form
    *_both("gen_small_357", (2, 3, 5, 7), (3, 1, None, 2, 3, 1), mix="mixed", final=True),
    Case("gen_small_6912", (1, 6, 9, 12), (None, 1, 2, 3, 1)),                          # 648 positions: a partial last block of 256
    Case("gen_small_1", (3, 1, 1, 1), (3, 1, 2), mix="mixed", rot=2, final=True),
    Case("gen_wide", (1, 1, 2, 904), (3, 2, None, 3, 1, 2, 3, 2)),                      # 17 * 904 * 4 > 60 KiB and 226 does not divide 256
]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
for _inv in (False, True):
    _reached = {dispatch(c, _inv) for c in CASES}
    assert _reached == TUPLES, (_inv, sorted(TUPLES - _reached, key=str), sorted(_reached - TUPLES, key=str))
assert dispatch(BY_NAME["gen_wide"]) == ("general", None, None, None) and 17 * 904 * 4 > LDS_CAP and 256 % 226
assert all(dispatch(c, i) == ("rows", None, None, None) for c in CASES if c.mis for i in (False, True))
assert dispatch(BY_NAME["rows_mis_zx"], True, z_none=True)[0] == dispatch(BY_NAME["rows_mis_bs"], True, z_none=True)[0] == "rows4"
for _form in ("rows4", "rows", "general"):      # all four clamp kinds, pre_scale 0.1, a stage without s, one without t: in every form
    _sel = [(c, k) for c in CASES if dispatch(c)[0] == _form for k in range(len(c.axes))]
    assert {c.param(k)[0] for c, k in _sel if c.has_s(k)} == {"NONE", "ATAN", "TANH", "SIGMOID"}, _form
    assert any(c.param(k)[2] == PRE01 for c, k in _sel) and any(not c.has_s(k) for c, k in _sel) and any(not c.has_t(k) for c, k in _sel), _form
    assert {3, 2, 1, None} <= {a for c in CASES if dispatch(c)[0] == _form for a in c.axes}, _form
assert sum(c.final for c in CASES) * 2 >= len(CASES) - 2                      # final_perm in (about) half the cases
assert all(math.prod(c.shape) * 2 <= 100_000 for c in CASES)
assert BY_NAME["r4_64_dead"].has_s(MIS_K) and BY_NAME["r4_64_dead"].has_t(MIS_K)


# ------------------------------------------------------------------------------------------------ the bound
def clamp_err(kind, clamp, pre):
    """absolute error of the clamped s (module docstring)"""
    A = RAW_MAX * pre
    a_kind = {"ATAN": 0.636 * ATAN_ERR, "TANH": TANH_ERR, "SIGMOID": (7 + A / 2) * U, "NONE": 2 * A * U}[kind]
    return clamp * a_kind


def stage_budget(st, fast_exp):
    if st.get("s_raw") is None:
        return 2 * U if st.get("t") is not None else 0.0
    return clamp_err(st["kind"], st["clamp"], st["pre"]) + (S_MAX * LOG2E * bool(fast_exp) + 4) * U


def value_bound(stages, form):
    return sum(stage_budget(st, form == "rows4") for st in stages) + 2 * U


def case_stage_params(c):
    return [{"s_raw": True if c.has_s(k) else None, "t": True if c.has_t(k) else None, "kind": c.param(k)[0], "clamp": c.param(k)[1],
             "pre": c.param(k)[2]} for k in range(len(c.axes))]


assert all(value_bound(case_stage_params(c), "rows4") < 1e-5 for c in CASES)
assert value_bound([], "rows4") == 2 * U


# ------------------------------------------------------------------------------------------------ inputs and references
_INPUTS, _REF = {}, {}


def inputs(c):
    """seeded fp32 CPU tensors: x [B,2C,H,W], z and low [B,C,H,W] for the inverse, the stage dicts of chain_ref, final_perm"""
    key = c.data or c.name
    if key in _INPUTS:
        return _INPUTS[key]
    B, Cc, H, W = c.shape
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    t = {"x": torch.randn(B, 2 * Cc, H, W, generator=g), "z": torch.randn(c.shape, generator=g), "low": torch.randn(c.shape, generator=g)}
    stages = []
    for k, ax in enumerate(c.axes):
        kind, clamp, pre = c.param(k)
        stages.append({"s_raw": torch.randn(c.shape, generator=g).clamp_(-RAW_MAX, RAW_MAX) if c.has_s(k) else None,
                       "t": torch.randn(c.shape, generator=g) if c.has_t(k) else None,
                       "perm": None if ax is None else torch.randperm([0, Cc, H, W][ax], generator=g), "axis": ax,
                       "kind": kind, "clamp": clamp, "pre": pre, "neg": k == len(c.axes) - 1})
    t["stages"] = stages
    t["final_perm"] = torch.randperm(Cc, generator=g) if c.final else None
    for st in stages:
        s = R.stage_s(st)
        assert s is None or float(s.abs().max()) <= S_MAX
    _INPUTS[key] = t
    return t


def reference(c, what):
    """float64, once per data set: "fwd" -> (z, low, logdet, M, sum|s|); "inv" / "inv0" (z = None) -> (x, logdet, M, sum|s|)"""
    key = (c.data or c.name, what)
    if key not in _REF:
        t = inputs(c)
        sabs = R.sum_abs_s(t["stages"], t["low"])
        if what == "fwd":
            z, low, ld, _ = R.chain_fwd(t["x"], t["stages"], t["final_perm"])
            _REF[key] = (z, low, ld, R.chain_magnitude(t["stages"], x=t["x"], final_perm=t["final_perm"]), sabs)
        else:
            zin = t["z"] if what == "inv" else None
            x, ld = R.chain_inv(zin, t["low"], t["stages"])
            _REF[key] = (x, ld, R.chain_magnitude(t["stages"], z=zin, low=t["low"], inverse=True), sabs)
    return _REF[key]


def rel_to_scale(got, ref, M):
    d = (torch.as_tensor(got).double().cpu() - ref).abs()
    return float((d / M.clamp_min(1e-300)).max())


def check_values(what, got, ref, M, bound):
    e = rel_to_scale(got, ref, M)
    print(f"[chain] {what}: e = {e:.3e} (bound {bound:.3e})")
    assert bool(torch.isfinite(torch.as_tensor(got)).all()), f"{what}: a NaN / Inf in the output"
    assert e <= bound, f"{what}: max |got - ref| / M = {e:.3e} > {bound:.3e}"
    return e


def check_logdet(what, got, init, ref_ld, sabs):
    err = (got.double().cpu() - init.double().cpu() - ref_ld).abs()
    lim = 8 * U * sabs
    print(f"[chain] {what}: log-det error {float(err.max()):.3e} (bound {float(lim.max()):.3e})")
    assert bool((err <= lim).all()), f"{what}: log-det off by {err.tolist()} > {lim.tolist()}"


def low_fp32(x):
    """the fp32 (e + o) * fl(1 / sqrt 2) of the kernels, on the CPU"""
    return (x[:, 0::2] + x[:, 1::2]) * torch.tensor(0.70710678118654752440, dtype=torch.float32)


def within_one_ulp(got, ref):
    got = got.cpu()
    ulp = torch.maximum(torch.nextafter(ref, torch.full_like(ref, math.inf)) - ref, ref - torch.nextafter(ref, torch.full_like(ref, -math.inf)))
    return bool(((got - ref).abs() <= ulp).all())


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ device layouts and launches
def sliced(t, before, after, off=0, pad=0):
    """t on the device as the channel slice [before, before + C) of a NaN-filled tensor that starts ``off`` floats into its allocation
    and has ``pad`` NaN floats between its samples (so the batch stride is (before + C + after) H W + pad)"""
    B, Cc, H, W = t.shape
    per = (before + Cc + after) * H * W + pad
    flat = torch.full((B * per + 4,), NAN, device="cuda")
    v = flat.as_strided((B, Cc, H, W), (per, H * W, W, 1), off + before * H * W)
    v.copy_(t)
    return v


class Dev:
    """the case's inputs on the device as channel slices between NaN channels (batch strides above their channel counts); the
    operand named by c.mis starts one float past a 16-byte boundary"""

    def __init__(self, c):
        t = inputs(c)
        m = c.mis
        self.c = c
        self.x = sliced(t["x"], 1, 2, off=int(m == "zx"), pad=2 * int(m == "bs"))
        self.z = sliced(t["z"], 2, 1, off=int(m == "zx"), pad=2 * int(m == "bs"))
        self.low = sliced(t["low"], 1, 1, off=int(m == "low"))
        self.s, self.t, self.perms = [], [], []
        for k, r in enumerate(t["stages"]):
            self.s.append(None if r["s_raw"] is None else sliced(r["s_raw"], 1, 2, off=int(m == "s" and k == MIS_K)))
            self.t.append(None if r["t"] is None else sliced(r["t"], 2, 1, off=int(m == "t" and k == MIS_K)))
            self.perms.append((None if r["perm"] is None else r["perm"].cuda(), r["axis"] or 1))
        self.ref_stages = t["stages"]
        self.fp = None if t["final_perm"] is None else t["final_perm"].cuda()

    def stages(self, sl=slice(None)):
        from cwfa_amd import ops
        out = []
        for k, r in enumerate(self.ref_stages):
            out.append(ops.stage(None if self.s[k] is None else self.s[k][sl], None if self.t[k] is None else self.t[k][sl], r["kind"], r["clamp"],
                                 pre_scale=r["pre"], t_neg_div_sqrt2=r["neg"], perm=self.perms[k][0], axis=self.perms[k][1]))
        return out

    def tables(self, inv):
        from cwfa_amd import ops
        return ops.chain_tables(self.perms, None if inv else self.fp, *self.c.shape[1:], "cuda")


def _bs(t):
    return t.stride(0)


def _aligned(tensors, stages):
    ok = all(t.data_ptr() % 16 == 0 and _bs(t) % 4 == 0 for t in tensors if t is not None)
    for st, _ in stages:
        ok = ok and (not st.s_raw or (st.s_raw % 16 == 0 and st.s_bs % 4 == 0)) and (not st.t or (st.t % 16 == 0 and st.t_bs % 4 == 0))
    return ok


def _form_of(c, tensors, stages):
    """the selection on the operands as they are: it must be the one the case stands for"""
    W, n = c.shape[3], len(c.axes)
    if rows4_shape(W) and _aligned(tensors, stages):
        return "rows4"
    return "rows" if W >= 64 and (2 * n + 1) * W * 4 <= LDS_CAP else "general"


def run_fwd(d, s=None, tables=None, ld=None, sq=None):
    """cwfa_chain_fwd_f32 itself, the outputs channel slices of NaN-filled tensors -> (z, low, form)"""
    from cwfa_amd import _lib, ops
    c = d.c
    sl = slice(None) if s is None else slice(s, s + 1)
    x = d.x[sl]
    B, Cc, H, W = (x.shape[0],) + c.shape[1:]
    stages = d.stages(sl)
    ch, keep = ops._chain(stages, tables)
    low, lflat = nan_around((B, Cc, H, W), 1, 2, off=int(c.mis == "low"))
    z, zflat = nan_around((B, Cc, H, W), 2, 1, off=int(c.mis == "out"))
    rc = _lib.lib().cwfa_chain_fwd_f32(ops._p(x), ops._p(low), ops._p(z), C.byref(ch), ops._p(d.fp), B, Cc, H, W, _bs(x), _bs(low), _bs(z),
                                       ops._p(ld), ops._p(sq), ops._stream())
    assert rc == 0, (c.name, rc)
    torch.cuda.synchronize()
    assert untouched_outside(low, lflat) and untouched_outside(z, zflat), (c.name, "a store outside the output slices")
    assert not bool(torch.isnan(low).any()) and not bool(torch.isnan(z).any()), (c.name, "a NaN neighbour was read or an element left out")
    return z, low, _form_of(c, [x, low, z], stages)


def run_inv(d, s=None, tables=None, ld=None, z_none=False):
    """cwfa_chain_inv_f32 itself -> (x, form)"""
    from cwfa_amd import _lib, ops
    c = d.c
    sl = slice(None) if s is None else slice(s, s + 1)
    z, low = None if z_none else d.z[sl], d.low[sl]
    B, Cc, H, W = (low.shape[0],) + c.shape[1:]
    stages = d.stages(sl)
    ch, keep = ops._chain(stages, tables)
    x, xflat = nan_around((B, 2 * Cc, H, W), 1, 1, off=int(c.mis == "out"))
    rc = _lib.lib().cwfa_chain_inv_f32(ops._p(z), ops._p(low), ops._p(x), C.byref(ch), B, Cc, H, W, 0 if z is None else _bs(z), _bs(low), _bs(x),
                                       ops._p(ld), ops._stream())
    assert rc == 0, (c.name, rc)
    torch.cuda.synchronize()
    assert untouched_outside(x, xflat), (c.name, "a store outside the output slice")
    assert not bool(torch.isnan(x).any()), (c.name, "a NaN neighbour was read or an element left out")
    return x, _form_of(c, [low, x, z], stages)


def _ld_init(B):
    return torch.tensor([0.75, -1.25, 2.5][:B], dtype=torch.float64, device="cuda")


def _ld_close(a, b, sabs):
    """log-dets of two launches of the same arithmetic: only the order of the double atomics differs"""
    return bool(((a.cpu() - b.cpu()).abs() <= 1e-12 * (sabs + 1.0)).all())


# ------------------------------------------------------------------------------------------------ the chains
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_chain_fwd_launch_vs_float64(c):
    from cwfa_amd import ops
    d = Dev(c)
    t = inputs(c)
    B = c.shape[0]
    zr, lowr, ldr, M, sabs = reference(c, "fwd")
    form = dispatch(c)[0]
    bound = value_bound(t["stages"], form)
    tabs = d.tables(False) if c.tables else None
    ld0, sq0 = _ld_init(B), torch.tensor([3.5], dtype=torch.float64, device="cuda")
    ld, sq = ld0.clone(), sq0.clone()
    z, low, got_form = run_fwd(d, tables=tabs, ld=ld, sq=sq)
    assert got_form == form, (c.name, "the layout does not give the form the case stands for", got_form, form)
    check_values(f"fwd {c.name} [{form}] z", z, zr, M, bound)
    l32 = low_fp32(t["x"])
    assert within_one_ulp(low, l32), (c.name, "low is more than one ulp from the fp32 (e + o) / sqrt 2")
    assert float((l32.double() - lowr).abs().max()) <= 2 * U * float(lowr.abs().max() + 1)
    check_logdet(f"fwd {c.name} [{form}]", ld, ld0, ldr, sabs)
    own = float((z.double() ** 2).sum())
    assert abs(float(sq) - 3.5 - own) <= 1e-12 * (own + 3.5), (c.name, "sumsq", float(sq) - 3.5, own)
    # without log-det and sumsq nothing else changes; with only one of them neither
    z2, low2, _ = run_fwd(d, tables=tabs)
    assert torch.equal(z2, z) and torch.equal(low2, low), (c.name, "logdet=None changed the values")
    ld1 = ld0.clone()
    z2, _, _ = run_fwd(d, tables=tabs, ld=ld1)
    assert torch.equal(z2, z) and _ld_close(ld1, ld, sabs)
    if c.tables:                                              # the composed tables against the dependent walk
        ldw = ld0.clone()
        zw, loww, _ = run_fwd(d, ld=ldw)
        assert torch.equal(zw, z) and torch.equal(loww, low) and _ld_close(ldw, ld, sabs), (c.name, "tables vs walk")
    for s in range(B):                                        # each sample alone
        lds = ld0.clone()
        zs, lows, _ = run_fwd(d, s=s, tables=tabs, ld=lds[s:s + 1])
        assert torch.equal(zs, z[s:s + 1]) and torch.equal(lows, low[s:s + 1]), (c.name, "sample", s)
        assert _ld_close(lds[s:s + 1], ld[s:s + 1], sabs[s:s + 1])
    # the tensor-level wrapper (dense outputs of its own)
    ldo, sqo = ld0.clone(), sq0.clone()
    zo, lowo = ops.chain_fwd(d.x, d.stages(), d.fp, logdet=ldo, sumsq=sqo, tables=tabs)
    if c.mis in ("low", "out"):                               # its outputs are aligned: the 16-byte form
        check_values(f"fwd {c.name} through ops [rows4] z", zo, zr, M, value_bound(t["stages"], "rows4"))
    else:
        assert torch.equal(zo, z) and _ld_close(ldo, ld, sabs) and abs(float(sqo) - float(sq)) <= 1e-12 * float(sq)
    assert torch.equal(lowo, low)


@pytest.mark.parametrize("z_none", [False, True], ids=["z", "z_none"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_chain_inv_launch_vs_float64(c, z_none):
    from cwfa_amd import ops
    d = Dev(c)
    t = inputs(c)
    B = c.shape[0]
    xr, ldr, M, sabs = reference(c, "inv0" if z_none else "inv")
    form = dispatch(c, True, z_none)[0]
    bound = value_bound(t["stages"], form)
    tabs = d.tables(True) if c.tables else None
    ld0 = _ld_init(B)
    ld = ld0.clone()
    x, got_form = run_inv(d, tables=tabs, ld=ld, z_none=z_none)
    assert got_form == form, (c.name, "the layout does not give the form the case stands for", got_form, form)
    check_values(f"inv {c.name} [{form}] z_none={z_none} x", x, xr, M, bound)
    check_logdet(f"inv {c.name} [{form}]", ld, ld0, ldr, sabs)
    x2, _ = run_inv(d, tables=tabs, z_none=z_none)
    assert torch.equal(x2, x), (c.name, "logdet=None changed the values")
    if c.tables:
        ldw = ld0.clone()
        xw, _ = run_inv(d, ld=ldw, z_none=z_none)
        assert torch.equal(xw, x) and _ld_close(ldw, ld, sabs), (c.name, "tables vs walk")
    for s in range(B):
        lds = ld0.clone()
        xs, _ = run_inv(d, s=s, tables=tabs, ld=lds[s:s + 1], z_none=z_none)
        assert torch.equal(xs, x[s:s + 1]), (c.name, "sample", s)
        assert _ld_close(lds[s:s + 1], ld[s:s + 1], sabs[s:s + 1])
    ldo = ld0.clone()
    xo = ops.chain_inv(None if z_none else d.z, d.low, d.stages(), logdet=ldo, tables=tabs)
    if c.mis == "out":
        check_values(f"inv {c.name} through ops [rows4] x", xo, xr, M, value_bound(t["stages"], "rows4"))
    else:
        assert torch.equal(xo, x) and _ld_close(ldo, ld, sabs)
    if z_none:                                                # z = None is z = zeros
        zero = Dev(c)
        zero.z.zero_()
        xz, zform = run_inv(zero, tables=tabs)
        assert zform != form or torch.equal(xz, x), (c.name, "z = None against z = zeros")


ROUND_TRIP = [c for c in CASES if not c.mis and not c.tables]


def _dense_stages(ref_stages):
    from cwfa_amd import ops
    return [ops.stage(None if r.get("s_raw") is None else r["s_raw"].cuda(), None if r.get("t") is None else r["t"].cuda(), r.get("kind", "ATAN"),
                      r.get("clamp", 2.0), pre_scale=r.get("pre", 1.0), t_neg_div_sqrt2=r.get("neg", False),
                      perm=None if r.get("perm") is None else r["perm"].cuda(), axis=r.get("axis") or 1) for r in ref_stages]


@pytest.mark.parametrize("c", ROUND_TRIP, ids=[c.name for c in ROUND_TRIP])
def test_round_trip_on_the_device(c):
    """chain_inv(chain_fwd(x)) with the reversed stages and the inverse gathers (final_perm: a leading stage that only gathers, so
    eight stages with a final permutation would be nine -- the eight-stage cases have none)"""
    from cwfa_amd import ops
    t = inputs(c)
    d = Dev(c)
    B = c.shape[0]
    zr, lowr, _, _, sabs = reference(c, "fwd")
    inv_ref = R.inverse_stages(t["stages"], t["final_perm"])
    assert len(inv_ref) <= 8
    ld0 = _ld_init(B)
    ld = ld0.clone()
    z, low = ops.chain_fwd(d.x, d.stages(), d.fp, logdet=ld)
    back = ops.chain_inv(z, low, _dense_stages(inv_ref), logdet=ld)
    torch.cuda.synchronize()
    M = R.chain_magnitude(inv_ref, z=zr, low=lowr, inverse=True)
    f_form, i_form = dispatch(c)[0], dispatch(Case("inv", c.shape, tuple(r.get("axis") for r in inv_ref)), True)[0]
    bound = value_bound(t["stages"], f_form) + value_bound(inv_ref, i_form)
    check_values(f"round trip {c.name} [{f_form} / {i_form}]", back, t["x"].double(), M, bound)
    err = (ld.cpu() - ld0.cpu()).abs()
    print(f"[chain] round trip {c.name}: log-dets cancel to {float(err.max()):.3e} (bound {float((8 * U * sabs).max()):.3e})")
    assert bool((err <= 8 * U * sabs).all()), (c.name, err.tolist())


MIS = [c for c in CASES if c.mis]


@pytest.mark.parametrize("inv", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("c", MIS, ids=[c.name for c in MIS])
def test_row_staged_against_16_byte_form(c, inv):
    """the same data through the row-staged form (one misaligned operand) and through the 16-byte form: each within its bound of
    float64 and within twice the bound of the other; low is identical"""
    base = BY_NAME["r4_64_dead"]
    t = inputs(c)
    assert inputs(base) is t
    da, db = Dev(base), Dev(c)
    b4, br = value_bound(t["stages"], "rows4"), value_bound(t["stages"], "rows")
    if inv:
        xr, _, M, _ = reference(c, "inv")
        (xa, fa), (xb, fb) = run_inv(da), run_inv(db)
        assert (fa, fb) == ("rows4", "rows")
        check_values(f"inv {base.name} [rows4]", xa, xr, M, b4)
        check_values(f"inv {c.name} [rows]", xb, xr, M, br)
        check_values(f"inv {c.name} [rows] vs [rows4]", xb, xa.double().cpu(), M, 2 * min(b4, br))
    else:
        zr, _, _, M, _ = reference(c, "fwd")
        (za, lowa, fa), (zb, lowb, fb) = run_fwd(da), run_fwd(db)
        assert (fa, fb) == ("rows4", "rows")
        check_values(f"fwd {base.name} [rows4]", za, zr, M, b4)
        check_values(f"fwd {c.name} [rows]", zb, zr, M, br)
        check_values(f"fwd {c.name} [rows] vs [rows4]", zb, za.double().cpu(), M, 2 * min(b4, br))
        assert torch.equal(lowa, lowb), "low differs between the forms"


# ------------------------------------------------------------------------------------------------ one stage: cwfa_affine_f32
def _affine_stage(shape, kind, ax, seed, gin=False):
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(seed)
    clamp, pre = {"NONE": (0.5, 1.0), "ATAN": (2.0, 1.0), "TANH": (2.0, PRE01), "SIGMOID": (1.5, 1.0)}[kind]
    return {"s_raw": torch.randn(shape, generator=g).clamp_(-RAW_MAX, RAW_MAX), "t": torch.randn(shape, generator=g),
            "perm": None if ax is None else torch.randperm([0, Cc, H, W][ax], generator=g), "axis": ax, "kind": kind, "clamp": clamp, "pre": pre,
            "neg": False, "gin": gin}


def _affine_dev(r, s_off=1):
    from cwfa_amd import ops
    return ops.stage(None if r["s_raw"] is None else sliced(r["s_raw"], s_off, 1), None if r["t"] is None else sliced(r["t"], 1, 2), r["kind"], r["clamp"],
                     pre_scale=r["pre"], t_neg_div_sqrt2=r["neg"], perm=None if r["perm"] is None else r["perm"].cuda(), axis=r["axis"] or 1,
                     gin=r.get("gin", False))


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("kind", ["NONE", "ATAN", "TANH", "SIGMOID"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 16, 64)])
def test_affine_vs_float64(shape, kind, rev):
    from cwfa_amd import ops
    B = shape[0]
    g = torch.Generator().manual_seed(sum(shape) + rev)
    x = torch.randn(shape, generator=g)
    xd = sliced(x, 2, 1)
    sign = -1.0 if rev else 1.0
    for ax in (None, 1, 2, 3):
        r = _affine_stage(shape, kind, ax, 7 * sum(shape) + (ax or 0))
        st = _affine_dev(r)
        bound = stage_budget(r, False)
        yr, ldr = R.affine(x, r, rev)
        sabs = R.stage_s(r).abs().flatten(1).sum(1)
        ld0, sq0 = _ld_init(B), torch.tensor([1.5], dtype=torch.float64, device="cuda")
        ld, sq = ld0.clone(), sq0.clone()
        out, flat = nan_around(shape, 1, 2)
        y = ops.affine(xd, st, rev, logdet=ld, sumsq=sq, out=out)
        torch.cuda.synchronize()
        assert y.data_ptr() == out.data_ptr() and untouched_outside(out, flat)
        check_values(f"affine {shape} {kind} rev={rev} axis={ax}", y, yr, R.affine_magnitude(x, r, rev), bound)
        check_logdet(f"affine {shape} {kind} rev={rev} axis={ax}", ld, ld0, ldr, sabs)
        assert bool((sign * (ld - ld0).cpu() * R.stage_s(r).flatten(1).sum(1).sign() >= 0).all()), "sign of the log-det"
        own = float((y.double() ** 2).sum())
        assert abs(float(sq) - 1.5 - own) <= 1e-12 * (own + 1.5)
        assert torch.equal(ops.affine(xd, st, rev), y), "logdet=None / a dense output changed the values"
        # x = None with a shape: the stage applied to zeros
        y0 = ops.affine(None, st, rev, shape=shape)
        check_values(f"affine {shape} {kind} rev={rev} axis={ax} x=None", y0, R.affine(None, r, rev, shape=shape)[0],
                     R.affine_magnitude(None, r, rev, shape=shape), bound)
        if ax is None:                                        # in place
            xc = xd.clone()
            assert ops.affine(xc, st, rev, out=xc) is xc and torch.equal(xc, y)
    # s only, t only
    r = _affine_stage(shape, kind, 3, 11)
    for drop in ("s_raw", "t"):
        r1 = dict(r, **{drop: None})
        check_values(f"affine {shape} {kind} rev={rev} without {drop}", ops.affine(xd, _affine_dev(r1), rev), R.affine(x, r1, rev)[0],
                     R.affine_magnitude(x, r1, rev), stage_budget(r1, False))
    # t_neg_div_sqrt2
    r1 = dict(r, neg=True)
    check_values(f"affine {shape} {kind} rev={rev} t = -t / sqrt 2", ops.affine(xd, _affine_dev(r1), rev), R.affine(x, r1, rev)[0],
                 R.affine_magnitude(x, r1, rev), stage_budget(r1, False))


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 16, 64)])
def test_affine_gin_vs_float64(shape, rev):
    """the GIN stage: the channel mean of the clamped s is removed at every pixel; the launch is given no log-det pointer, so a
    log-det handed to cwfa_affine_f32 stays bit for bit what it was (the stage's log-det is zero)"""
    from cwfa_amd import ops
    B, Cc = shape[:2]
    g = torch.Generator().manual_seed(sum(shape) + 20 + rev)
    x = torch.randn(shape, generator=g)
    xd = sliced(x, 1, 1)
    for ax in (None, 1, 2, 3):
        r = _affine_stage(shape, "ATAN", ax, 90 + (ax or 0), gin=True)
        yr, ldr = R.affine(x, r, rev)
        assert float(ldr.abs().max()) <= 1e-12
        ld0, sq = _ld_init(B), torch.tensor([0.25], dtype=torch.float64, device="cuda")
        ld = ld0.clone()
        out, flat = nan_around(shape, 2, 1)
        y = ops.affine(xd, _affine_dev(r), rev, logdet=ld, sumsq=sq, out=out)
        torch.cuda.synchronize()
        assert untouched_outside(out, flat)
        check_values(f"affine GIN {shape} rev={rev} axis={ax}", y, yr, R.affine_magnitude(x, r, rev), stage_budget(r, False) + (Cc + 3) * S_MAX * U)
        assert torch.equal(ld, ld0), "the GIN launch touched the log-det"
        own = float((y.double() ** 2).sum())
        assert abs(float(sq) - 0.25 - own) <= 1e-12 * (own + 0.25)
        # the mean matters: the same stage without the GIN flag is far away
        plain = dict(r, gin=False)
        assert rel_to_scale(ops.affine(xd, _affine_dev(plain), rev), yr, R.affine_magnitude(x, r, rev)) > 1e-3


# ------------------------------------------------------------------------------------------------ cwfa_channel_affine_f32
@pytest.mark.parametrize("perm", ["none", "in", "out"])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (16, 16), (1, 257)])
def test_channel_affine_vs_float64(hw, inverse, perm):
    from cwfa_amd import ops
    B, Cc = 2, 5
    shape = (B, Cc) + hw
    g = torch.Generator().manual_seed(hw[0] * hw[1] + 2 * inverse)
    x = torch.randn(shape, generator=g)
    sc = torch.rand(Cc, generator=g) + 0.5
    sc[1] = -sc[1]
    sh = torch.randn(Cc, generator=g)
    p = torch.randperm(Cc, generator=g)
    kw = {"none": {}, "in": {"perm_in": p}, "out": {"perm_out": p}}[perm]
    kwd = {k: v.cuda() for k, v in kw.items()}
    xd = sliced(x, 1, 2)                                       # a strided x
    for scale, shift in ((sc, sh), (None, sh), (sc, None), (None, None)):
        ref = R.channel_affine(x, scale, shift, inverse, **kw)
        one, zero = torch.ones(Cc), torch.zeros(Cc)
        M = R.channel_affine(x.abs(), (one if scale is None else scale).abs(), -(zero if shift is None else shift).abs() if inverse else
                             (zero if shift is None else shift).abs(), inverse, **kw)
        got = ops.channel_affine(xd, None if scale is None else scale.cuda(), None if shift is None else shift.cuda(), inverse, **kwd)
        check_values(f"channel_affine HW={hw} inverse={inverse} perm={perm} scale={scale is not None} shift={shift is not None}", got, ref, M, 2 * U)
        assert torch.equal(got, ops.channel_affine(x.cuda(), None if scale is None else scale.cuda(), None if shift is None else shift.cuda(),
                                                   inverse, **kwd)), "strided against dense x"
    if not inverse:                                            # mode 1 with the inverse permutation undoes mode 0
        y = ops.channel_affine(xd, sc.cuda(), sh.cuda(), False, **kwd)
        q = R.inverse_perm(p)
        # "out": y[c] = A_j(x[j]), j = p[c] -> channel j reads y[q[j]] with its own parameters: perm_in = q
        # "in":  y[c] = A_c(x[p[c]])        -> channel j = p[c] reads y[q[j]] with the parameters of q[j]: perm_out = q
        back_kw = {"none": {}, "in": {"perm_out": q.cuda()}, "out": {"perm_in": q.cuda()}}[perm]
        back = ops.channel_affine(y, sc.cuda(), sh.cuda(), True, **back_kw)
        ratio = sh.double().abs() / sc.double().abs()          # per channel whose parameters were applied
        scale_x = x.double().abs() + (ratio[q] if perm == "in" else ratio).view(1, Cc, 1, 1)
        check_values(f"channel_affine HW={hw} perm={perm} mode 1 undoes mode 0", back, x.double(), scale_x, 4 * U)


# ------------------------------------------------------------------------------------------------ rejected and empty calls
def _all_nan(*ts):
    torch.cuda.synchronize()
    return all(bool((t.view(torch.int32) == NAN_BITS).all()) for t in ts)


def test_rejected_and_empty_calls_launch_nothing():
    """nine stages, a GIN stage in a chain, a bad clamp kind, a bad gather axis: the error code and untouched outputs; B = 0 and
    C = 0: CWFA_OK and untouched outputs"""
    from cwfa_amd import _lib, ops
    L = _lib.lib()
    B, Cc, H, W = shape = (2, 2, 16, 64)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, 2 * Cc, H, W, generator=g).cuda()
    zin, lowin = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    s_raw, tt = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    perm = torch.randperm(W, generator=g).cuda()
    low, z = torch.full(shape, NAN, device="cuda"), torch.full(shape, NAN, device="cuda")
    xo = torch.full((B, 2 * Cc, H, W), NAN, device="cuda")
    ld0 = _ld_init(B)
    ld, sq = ld0.clone(), torch.tensor([3.5], dtype=torch.float64, device="cuda")
    n = Cc * H * W

    def fwd(ch, B=B, Cc=Cc):
        return L.cwfa_chain_fwd_f32(ops._p(x), ops._p(low), ops._p(z), C.byref(ch), None, B, Cc, H, W, 2 * n, n, n, ops._p(ld), ops._p(sq), ops._stream())

    def inv(ch, B=B, Cc=Cc):
        return L.cwfa_chain_inv_f32(ops._p(zin), ops._p(lowin), ops._p(xo), C.byref(ch), B, Cc, H, W, n, n, 2 * n, ops._p(ld), ops._stream())

    def aff(st, B=B, Cc=Cc):
        return L.cwfa_affine_f32(ops._p(zin), ops._p(z), C.byref(st), 0, B, Cc, H, W, n, n, ops._p(ld), ops._p(sq), ops._stream())

    good = ops.stage(s_raw, tt, perm=perm, axis=3)
    ok, keep = ops._chain([good] * 2)
    # nine stages
    with pytest.raises(ValueError):
        ops.chain_fwd(x, [good] * 9)
    with pytest.raises(ValueError):
        ops.chain_inv(zin, lowin, [good] * 9)
    nine, _ = ops._chain([good] * 8)
    nine.n_stages = 9
    assert fwd(nine) == -1 and inv(nine) == -1
    # a GIN stage in a chain
    gin, _ = ops._chain([good, ops.stage(s_raw, tt, gin=True)])
    assert fwd(gin) == -1 and inv(gin) == -1
    with pytest.raises(_lib.CwfaHipError, match=r"code -1\)"):
        ops.chain_fwd(x, [good, ops.stage(s_raw, tt, gin=True)])
    # a bad clamp kind, a bad gather axis (chains and the single stage)
    for field, value in (("clamp_kind", 4), ("clamp_kind", -1), ("perm_axis", 0), ("perm_axis", 4)):
        st, _ = ops.stage(s_raw, tt, perm=perm, axis=3)
        setattr(st, field, value)
        bad, _ = ops._chain([good, (st, ())])
        assert fwd(bad) == -1 and inv(bad) == -1 and aff(st) == -1, (field, value)
    # empty problems
    for kw in ({"B": 0}, {"Cc": 0}):
        assert fwd(ok, **kw) == 0 and inv(ok, **kw) == 0 and aff(good[0], **kw) == 0, kw
    assert _all_nan(low, z, xo), "a rejected or empty call wrote an output"
    assert torch.equal(ld, ld0) and float(sq) == 3.5
    # channel affine: both permutations together
    y = torch.full(shape, NAN, device="cuda")
    p2 = torch.randperm(Cc, generator=g).cuda()
    assert L.cwfa_channel_affine_f32(ops._p(zin), ops._p(y), None, None, 0, ops._p(p2), ops._p(p2), B, Cc, H * W, n, n, ops._stream()) == -1
    assert L.cwfa_channel_affine_f32(ops._p(zin), ops._p(y), None, None, 2, None, None, B, Cc, H * W, n, n, ops._stream()) == -1
    with pytest.raises(_lib.CwfaHipError, match=r"code -1\)"):
        ops.channel_affine(zin, None, None, perm_in=p2, perm_out=p2)
    for b_, c_, hw_ in ((0, Cc, H * W), (B, 0, H * W), (B, Cc, 0)):
        assert L.cwfa_channel_affine_f32(ops._p(zin), ops._p(y), None, None, 0, None, None, b_, c_, hw_, n, n, ops._stream()) == 0
    assert _all_nan(y)
    # the same calls are accepted once they are well formed
    assert fwd(ok) == 0 and inv(ok) == 0 and aff(good[0]) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(low).any() | torch.isnan(z).any() | torch.isnan(xo).any())


# ------------------------------------------------------------------------------------------------ CPU only: the harness on fp32 arithmetic
def _fp32_chain(t, inv, z_none=False):
    """the chains in plain fp32 torch on the CPU (expf, atan of libm): what a correct kernel computes up to its own function errors"""
    f = torch.float32
    c = torch.tensor(0.70710678118654752440, dtype=f)

    def st_s(st):
        if st["s_raw"] is None:
            return None
        a = st["s_raw"] * torch.tensor(st["pre"], dtype=f)
        k = st["kind"]
        cl = torch.tensor(st["clamp"], dtype=f)
        return cl * (torch.tensor(0.636, dtype=f) * torch.atan(a)) if k == "ATAN" else cl * torch.tanh(a) if k == "TANH" else \
            cl * (2 * (1 / (1 + torch.exp(-a)) - 0.5)) if k == "SIGMOID" else cl * a

    def st_t(st):
        if st["t"] is None:
            return None
        return (-st["t"]) / torch.tensor(math.sqrt(2.0), dtype=f) if st["neg"] else st["t"] * torch.tensor(st["pre"], dtype=f)

    if not inv:
        v = (t["x"][:, 0::2] - t["x"][:, 1::2]) * c
    else:
        v = torch.zeros_like(t["low"]) if z_none else t["z"]
    for st in t["stages"]:
        if st["perm"] is not None:
            v = v.index_select(st["axis"], st["perm"])
        s, tt = st_s(st), st_t(st)
        s = torch.zeros_like(v) if s is None else s
        tt = torch.zeros_like(v) if tt is None else tt
        v = (v - tt) * torch.exp(-s) if inv else torch.exp(s) * v + tt
    if not inv:
        return v if t["final_perm"] is None else v.index_select(1, t["final_perm"])
    x = torch.empty(t["x"].shape)
    x[:, 0::2], x[:, 1::2] = (t["low"] + v) * c, (t["low"] - v) * c
    return x


if __name__ == "__main__":
    worst = {}
    for c_ in CASES:
        t_ = inputs(c_)
        for inv_, zn_ in ((False, False), (True, False), (True, True)):
            refs = reference(c_, "fwd" if not inv_ else "inv0" if zn_ else "inv")
            ref_, M_ = refs[0], refs[3 if not inv_ else 2]
            form_ = dispatch(c_, inv_, zn_)[0]
            e_ = rel_to_scale(_fp32_chain(t_, inv_, zn_), ref_, M_)
            b_ = value_bound(t_["stages"], form_)
            print(f"{c_.name:18s} {'inv' if inv_ else 'fwd'} z_none={zn_:d} [{form_:7s}] fp32 on the CPU e = {e_:.3e}, bound {b_:.3e}")
            assert e_ <= b_
            worst[form_] = max(worst.get(form_, 0.0), e_)
    print(worst)
