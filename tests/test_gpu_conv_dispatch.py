"""GPU (MI355X): every launch configuration of the fp32 convolution kernels and of the split 1x1 GEMM against float64.

csrc/conv2d.hip, csrc/conv_wino.hip and csrc/conv_wino2d.hip pick among
  * 58 instantiations of conv2d_mfma_kernel<C, EPI, PRO> (11 tilings, each with its own set of specialised epilogues),
  * 16 of conv3x3_wino_kernel<W32|W64|W128, WEPI, PRO>,
  * 10 of conv3x3_wino2d_kernel<W2EPI, PRO, ALIGNED>,
  * 3 epilogues of conv1x1_split_kernel, each built for the three operand formats (9 paths).
`dispatch` below restates that selection from the host code; the case list is asserted (at import) to reach every tuple, so an
instantiation added later fails the import until it has a case.  Every case runs with
  * x, the skip tensor, the residual (and both sources of a two-source input) as channel slices of larger tensors whose other
    channels hold NaN: a read past the slice cannot hide behind the zero weights the banks are padded with;
  * the output as a channel slice of a NaN-filled tensor: nothing outside the slice may be written;
  * load-side prologues on the dyadic grid of test_gpu_split_dispatch.inputs (the fp32 prologue is exact, fused or not);
  * each sample alone bit-equal to its slice of the batched launch.
Bounds (the project's own): direct kernels 2e-6 (bias only) / 3e-6 (activation or residual), both Winograd forms 5e-6, the GEMM
5e-6 in split_bf16 and, in bf16 / fp16, check16 at 2e-5 against operands rounded as the kernel rounds them.

The 8-byte stores of EPI_UP depend on the output pointer only (a row of the shuffled output has 2 W floats, an even number for
every W), so the odd-W cases take them as well; the 4-byte fallback is reached by the cases whose output starts one float past an
8-byte boundary (``mis="y"``).

Every test prints its max-rel error next to the bound before it asserts (pytest -s).  Largest figure measured on an MI355X:
  direct       6.6e-7 bias only (c7_64_none; bound 2e-6), 1.0e-6 with an activation / residual (c7_32_pro_gen; 3e-6)
  Winograd     1-D 3.4e-7, 2-D 2.9e-7 (5e-6)
  GEMM         split_bf16 2.0e-7 (5e-6); bf16 1.3e-7, fp16 1.5e-7 (2e-5), the other format's reference >= 1.6e-3 away
  fused layer  (tape form) y 3.4e-7, hidden map 5.4e-7 (3e-6)
Every case passed the NaN-neighbour and the tail-store checks with the kernels as they stand: no kernel was changed."""
import ctypes as C
import zlib
from dataclasses import dataclass

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, rel_err
from split_ref import F16_TOL, _pro32, b16, check16, h, maxrel

pytestmark = pytest.mark.gpu
FORMATS = ("split_bf16", "bf16", "fp16")
SPLIT_TOL = 5e-6
DIRECT_TOL, DIRECT_EPI_TOL, WINO_TOL = 2e-6, 3e-6, 5e-6
NAN = float("nan")
NAN_BITS = int(torch.tensor([NAN]).view(torch.int32)[0])

# ------------------------------------------------------------------------------------------------ the host selection, restated
GEN, N, E, RE, P, RP, G, U, K = "GENERIC", "NONE", "ELU", "RES_ELU", "PRELU", "RES_PRELU", "GELU_RES", "UP", "NONE_BLK8"
CK = {1: 16, 3: 8, 7: 4}                                     # input channels per K chunk (direct kernels; Winograd: 8; GEMM: 16)

# launch<C, ALLOWED, ALLOWED_PRO> of cwfa_conv2d_f32: the specialised epilogues without / with a load-side prologue
_C1_32, _C1_64, _C1_128 = ({N, P, G}, {P}), ({N, RE, G, K}, set()), ({N, U, K}, {U})
LAUNCH = {"C3_32": ({N, P, RP}, set()), "C3_64": ({N, E, P, RP}, set()), "C3_128": ({N, P}, {P}),
          "C1_32": _C1_32, "C1_64": _C1_64, "C1_128": _C1_128, "C1v_32": _C1_32, "C1v_64": _C1_64, "C1v_128": _C1_128,
          "C7_32": ({N}, set()), "C7_64": ({N}, set())}
DIRECT_TUPLES = ({(t, e, False) for t, (a, _) in LAUNCH.items() for e in a | {GEN}}
                 | {(t, e, True) for t, (_, a) in LAUNCH.items() for e in a | {GEN}})
WINO_TUPLES = ({("W32", GEN, True), ("W64", GEN, True), ("W128", P, True), ("W128", GEN, True)}
               | {("W32", e, False) for e in (N, P, RP, GEN)} | {("W64", e, False) for e in (N, E, P, RP, GEN)}
               | {("W128", e, False) for e in (N, P, GEN)})
WINO2D_TUPLES = {(e, p, a) for e, p in ((P, True), (P, False), (N, False), (GEN, True), (GEN, False)) for a in (True, False)}
GEMM_TUPLES = {(e, f) for e in (N, U, GEN) for f in FORMATS}
assert (len(DIRECT_TUPLES), len(WINO_TUPLES), len(WINO2D_TUPLES), len(GEMM_TUPLES)) == (58, 16, 10, 9)


@dataclass(frozen=True)
class Case:
    name: str
    fam: str                  # "direct" | "wino" | "wino2d" | "gemm"
    ks: int
    cin: int                  # input channels (two-source input: of both sources together)
    cout: int                 # rows of the packed bank (transposed banks: 4 * Co)
    H: int
    W: int
    act: object = None
    res: bool = False
    act2: object = None
    pro: str = ""             # load-side prologue: "aff" ([B,Cin] tables), "aff1" ([Cin] tables), "add" (skip tensor), combined by "+"
    up: bool = False          # ConvTranspose2d(k2, s2) bank: the output is the shuffled [B, cout / 4, 2H, 2W]
    blk: bool = False         # out_blocked: [Cout/8][H][W][8]
    cat: int = 0              # two-source input: channels of the first source
    mis: str = ""             # "x" / "add" / "y": that tensor starts one float past a 16-byte boundary
    B: int = 2


def classify_epilogue(c):
    if c.blk:
        return K
    if c.up:
        return U if not c.res and c.act is None and c.act2 is None else GEN
    if not c.res and c.act2 is None and c.act in (None, "elu", "prelu"):
        return {None: N, "elu": E, "prelu": P}[c.act]
    if c.res and c.act is None and c.act2 in ("elu", "prelu"):
        return RE if c.act2 == "elu" else RP
    if c.res and c.act == "gelu" and c.act2 is None:
        return G
    return GEN


def rows16(c):
    """the `v4` predicate of cwfa_conv2d_f32 / `aligned` of cwfa_wino2d_conv, from the case: rows, batch strides (the layouts of Dev
    keep them multiples of four floats whenever W is) and the base pointers of x and the skip tensor on 16-byte boundaries"""
    return c.W % 4 == 0 and c.mis not in ("x", "add")


def packed_cin(c):
    return (c.cat + 15) // 16 * 16 + c.cin - c.cat if c.cat else c.cin


def nchunks(c):
    return -(-packed_cin(c) // (CK[c.ks] if c.fam == "direct" else 8 if c.ks == 3 else 16))


def dispatch(c):
    """the instantiation case c reaches: direct (tiling, EPI, PRO); Winograd 1-D (tiling, WEPI, PRO); 2-D (W2EPI, PRO, ALIGNED); GEMM EPI"""
    pro, cls = bool(c.pro), 0 if c.cout <= 32 else 1 if c.cout <= 64 else 2
    if c.fam == "gemm":                                       # cwfa_conv_split_f32
        epi = classify_epilogue(c)
        return epi if epi in (N, U) else GEN
    if c.fam == "direct":                                     # select_cfg + launch_sel
        size = ("32", "64", "128")[cls if c.ks != 7 else min(cls, 1)]
        tiling = {3: "C3_", 7: "C7_", 1: "C1v_" if rows16(c) else "C1_"}[c.ks] + size
        epi = classify_epilogue(c)
        return (tiling, epi if epi in LAUNCH[tiling][pro] else GEN, pro)
    plain = not c.res and c.act2 is None
    if c.fam == "wino2d":                                     # dispatch2d
        if plain and c.act == "prelu":
            return (P, pro, rows16(c))
        if plain and c.act is None and not pro:
            return (N, False, rows16(c))
        return (GEN, pro, rows16(c))
    epi = {None: N, "elu": E, "prelu": P}[c.act] if plain and c.act in (None, "elu", "prelu") else GEN      # cwfa_wino_conv
    if c.res and c.act is None and c.act2 == "prelu":
        epi = RP
    if cls == 0:
        return ("W32", GEN, True) if pro else ("W32", epi if epi in (N, P, RP) else GEN, False)
    if cls == 1:
        return ("W64", GEN, True) if pro else ("W64", epi, False)
    if pro:
        return ("W128", P if epi == P else GEN, True)
    return ("W128", epi if epi in (N, P) else GEN, False)


# ------------------------------------------------------------------------------------------------ cases
def D(name, ks, cin, cout, H, W, **kw):
    return Case(name, "direct", ks, cin, cout, H, W, **kw)


def Wn(name, cin, cout, H, W, **kw):
    return Case(name, "wino", 3, cin, cout, H, W, **kw)


def W2(name, cin, cout, H, W, **kw):
    return Case(name, "wino2d", 3, cin, cout, H, W, **kw)


def Gm(name, cin, cout, H, W, **kw):
    return Case(name, "gemm", 1, cin, cout, H, W, **kw)


CASES = [
    # ---- direct 3x3 (run with winograd_min_cout above every Cout); CK = 8: Cin 3 / 16 / 17 / 33 = 1 / 2 / 3 / 5 chunks
    D("c3_32_none", 3, 3, 7, 9, 33),
    D("c3_32_prelu", 3, 16, 32, 8, 31, act="prelu"),
    D("c3_32_res_prelu", 3, 17, 32, 17, 20, res=True, act2="prelu"),
    D("c3_32_gen", 3, 33, 7, 1, 32, act="elu", res=True, act2="gelu"),
    D("c3_32_pro_gen", 3, 16, 32, 9, 36, act="prelu", pro="aff+add"),
    D("c3_64_none", 3, 17, 33, 17, 33),
    D("c3_64_elu", 3, 3, 64, 8, 32, act="elu"),
    D("c3_64_prelu", 3, 33, 64, 9, 31, act="prelu"),
    D("c3_64_res_prelu", 3, 16, 33, 1, 36, res=True, act2="prelu"),
    D("c3_64_gen", 3, 16, 64, 17, 20, act="prelu", res=True, act2="relu"),
    D("c3_64_pro_gen", 3, 3, 33, 8, 33, pro="aff1"),
    D("c3_128_none", 3, 16, 65, 9, 33),
    D("c3_128_prelu", 3, 3, 129, 8, 20, act="prelu"),
    D("c3_128_gen", 3, 17, 129, 17, 31, act="gelu", res=True, act2="elu"),
    D("c3_128_pro_prelu", 3, 33, 65, 9, 32, act="prelu", pro="aff+add"),
    D("c3_128_pro_gen", 3, 16, 129, 1, 33, act="relu", res=True, pro="add"),
    # ---- direct 1x1, scalar-staged (W % 4 != 0); CK = 16: Cin 5, 16 / 17, 32 / 40 = 1 / 2 / 3 chunks
    D("c1_32_none", 1, 5, 7, 9, 33),
    D("c1_32_prelu", 1, 17, 32, 8, 31, act="prelu"),
    D("c1_32_gelu_res", 1, 40, 32, 17, 33, act="gelu", res=True),
    D("c1_32_gen", 1, 16, 7, 1, 31, act="relu", res=True, act2="prelu"),
    D("c1_32_pro_prelu", 1, 32, 32, 9, 33, act="prelu", pro="aff"),
    D("c1_32_pro_gen", 1, 17, 7, 8, 31, act="elu", pro="aff1+add"),
    D("c1_32_up_gen", 1, 16, 28, 9, 33, up=True),                               # (no EPI_UP on the smaller classes: generic)
    D("c1_64_none", 1, 17, 33, 9, 33),
    D("c1_64_res_elu", 1, 5, 64, 17, 31, res=True, act2="elu"),
    D("c1_64_gelu_res", 1, 32, 33, 8, 33, act="gelu", res=True),
    D("c1_64_blk8", 1, 40, 64, 9, 31, blk=True),
    D("c1_64_gen", 1, 16, 64, 1, 33, act="prelu", res=True, act2="gelu"),
    D("c1_64_pro_gen", 1, 40, 33, 9, 31, pro="aff"),
    D("c1_64_up_res", 1, 17, 64, 8, 33, up=True, res=True),                     # (the residual indexes the shuffled output)
    D("c1_128_none", 1, 40, 129, 9, 33),
    D("c1_128_up", 1, 17, 132, 8, 31, up=True),
    D("c1_128_blk8", 1, 16, 136, 9, 33, blk=True),
    D("c1_128_gen", 1, 5, 65, 17, 31, act="elu", res=True, act2="elu"),
    D("c1_128_pro_up", 1, 32, 68, 9, 33, up=True, pro="aff+add"),
    D("c1_128_pro_gen", 1, 17, 129, 8, 31, act="prelu", pro="aff1"),
    # ---- direct 1x1, vector-staged (W % 4 == 0, 16-byte aligned x / skip tensor)
    D("c1v_32_none", 1, 16, 32, 8, 32),
    D("c1v_32_prelu", 1, 5, 7, 17, 20, act="prelu"),
    D("c1v_32_gelu_res", 1, 32, 32, 9, 36, act="gelu", res=True),
    D("c1v_32_gen", 1, 40, 7, 9, 20, act="elu", res=True, act2="relu"),
    D("c1v_32_pro_prelu", 1, 17, 7, 1, 32, act="prelu", pro="add"),
    D("c1v_32_pro_gen", 1, 40, 32, 17, 36, act="gelu", res=True, act2="prelu", pro="aff+add"),
    D("c1v_32_up_res", 1, 5, 32, 8, 20, up=True, res=True),
    D("c1v_64_none", 1, 40, 64, 17, 32),
    D("c1v_64_res_elu", 1, 17, 33, 9, 20, res=True, act2="elu"),
    D("c1v_64_gelu_res", 1, 5, 64, 8, 36, act="gelu", res=True),
    D("c1v_64_blk8", 1, 16, 40, 9, 20, blk=True),
    D("c1v_64_gen", 1, 32, 33, 1, 36, act="relu", act2="elu"),
    D("c1v_64_pro_gen", 1, 16, 64, 8, 32, act="prelu", pro="aff1+add"),
    D("c1v_64_up_gen", 1, 32, 36, 9, 32, up=True),
    D("c1v_128_none", 1, 17, 65, 8, 36),
    D("c1v_128_up", 1, 40, 132, 9, 20, up=True),
    D("c1v_128_up_misy", 1, 16, 68, 8, 32, up=True, mis="y"),                   # (the 4-byte fallback of the EPI_UP stores)
    D("c1v_128_blk8", 1, 32, 72, 17, 32, blk=True),
    D("c1v_128_gen", 1, 16, 129, 9, 36, act="gelu", res=True, act2="gelu"),
    D("c1v_128_pro_up", 1, 5, 132, 8, 36, up=True, pro="aff+add"),
    D("c1v_128_pro_gen", 1, 32, 65, 9, 20, res=True, pro="add"),
    # ---- `v4` off by the pointer alone: W % 4 == 0, x (or only the skip tensor) one float past a 16-byte boundary
    D("c1_64_mis_x", 1, 32, 64, 8, 32, mis="x"),
    D("c1_64_mis_add", 1, 17, 33, 9, 36, pro="add", mis="add"),
    # ---- two-source input (cat=): c1 not a multiple of 16; 5 | 7: one chunk from each source
    D("c1_32_cat", 1, 12, 7, 9, 33, cat=5),
    D("c1v_32_cat", 1, 37, 32, 8, 32, act="prelu", cat=17),
    D("c1_64_cat", 1, 64, 33, 17, 31, res=True, act2="elu", cat=24),
    D("c1v_64_cat", 1, 21, 64, 9, 20, cat=5),
    # ---- direct 7x7; CK = 4: Cin 3, 4 / 6 / 13 = 1 / 2 / 4 chunks
    D("c7_32_none", 7, 3, 7, 9, 33),
    D("c7_32_none_1chunk", 7, 4, 32, 1, 36),
    D("c7_32_gen", 7, 6, 32, 8, 31, act="relu", res=True, act2="elu"),
    D("c7_32_pro_gen", 7, 13, 32, 17, 20, act="gelu", pro="aff+add"),
    D("c7_64_none", 7, 13, 33, 9, 33),
    D("c7_64_gen", 7, 4, 64, 17, 31, act="gelu", res=True, act2="prelu"),
    D("c7_64_pro_gen", 7, 3, 129, 8, 32, pro="aff1"),
    # ---- Winograd F(2,3), 64-column tiles
    Wn("w32_none", 3, 7, 9, 33),
    Wn("w32_prelu", 16, 32, 8, 65, act="prelu"),
    Wn("w32_res_prelu", 17, 32, 17, 20, res=True, act2="prelu"),
    Wn("w32_gen", 33, 7, 1, 31, act="elu", res=True, act2="relu"),
    Wn("w32_pro_gen", 17, 32, 9, 36, act="prelu", pro="aff+add"),
    Wn("w64_none", 16, 33, 17, 66),
    Wn("w64_elu", 33, 64, 8, 31, act="elu"),
    Wn("w64_prelu", 3, 64, 9, 32, act="prelu"),
    Wn("w64_res_prelu", 17, 33, 1, 33, res=True, act2="prelu"),
    Wn("w64_gen", 16, 64, 9, 20, act="gelu", res=True, act2="prelu"),
    Wn("w64_pro_gen", 33, 33, 8, 33, act="elu", pro="aff"),
    Wn("w128_none", 17, 65, 9, 65),
    Wn("w128_prelu", 16, 129, 8, 33, act="prelu"),
    Wn("w128_gen", 3, 129, 17, 31, act="relu", res=True, act2="gelu"),
    Wn("w128_pro_prelu", 33, 129, 9, 20, act="prelu", pro="aff1+add"),
    Wn("w128_pro_gen", 16, 65, 1, 36, act="prelu", res=True, act2="elu", pro="add"),
    # ---- Winograd F(2x2,3x3) (run with winograd_2d = 1): ALIGNED (W % 4 == 0, aligned x / skip tensor) and not
    W2("w2a_none", 16, 65, 9, 32),
    W2("w2a_prelu", 3, 129, 8, 20, act="prelu"),
    W2("w2a_gen", 17, 65, 17, 36, act="elu", res=True, act2="prelu"),
    W2("w2a_pro_prelu", 33, 129, 9, 32, act="prelu", pro="aff+add"),
    W2("w2a_pro_gen", 16, 65, 1, 20, pro="aff"),
    W2("w2u_none", 17, 129, 9, 66),
    W2("w2u_prelu", 16, 65, 17, 31, act="prelu"),
    W2("w2u_gen", 33, 129, 8, 33, act="gelu", res=True),
    W2("w2u_pro_prelu", 3, 65, 9, 33, act="prelu", pro="add"),
    W2("w2u_pro_gen", 17, 129, 8, 31, act="relu", res=True, act2="relu", pro="aff1+add"),
    W2("w2u_mis_x", 16, 65, 8, 32, mis="x"),
    W2("w2u_mis_add", 17, 129, 9, 36, act="prelu", pro="add", mis="add"),
    # ---- split 1x1 GEMM (every case in the three formats); CK = 16: Cin 5, 16 / 32 / 33 / 70 = 1 / 2 / 3 / 5 chunks
    Gm("g_none", 5, 129, 9, 33),
    Gm("g_none_pro", 32, 260, 8, 31, pro="aff"),
    Gm("g_gen", 16, 200, 17, 20, act="elu", res=True, act2="gelu"),
    Gm("g_gen_pro", 33, 256, 1, 32, act="prelu", res=True, act2="relu", pro="add"),
    Gm("g_gen_act", 70, 260, 9, 36, act="gelu", pro="aff1+add"),
    Gm("g_up", 16, 132, 8, 31, up=True),
    Gm("g_up_pro", 70, 260, 9, 20, up=True, pro="aff+add"),
    Gm("g_up_res", 32, 200, 8, 33, up=True, res=True),
    Gm("g_up_misy", 5, 256, 9, 32, up=True, mis="y"),
]
IDS = [c.name for c in CASES]
assert len(set(IDS)) == len(IDS)
FP32_CASES = [c for c in CASES if c.fam != "gemm"]
GEMM_CASES = [c for c in CASES if c.fam == "gemm"]


def _reached(fam):
    return {dispatch(c) for c in CASES if c.fam == fam}


assert _reached("direct") == DIRECT_TUPLES, (sorted(DIRECT_TUPLES - _reached("direct")), sorted(_reached("direct") - DIRECT_TUPLES))
assert _reached("wino") == WINO_TUPLES, (sorted(WINO_TUPLES - _reached("wino")), sorted(_reached("wino") - WINO_TUPLES))
assert _reached("wino2d") == WINO2D_TUPLES, sorted(WINO2D_TUPLES - _reached("wino2d"), key=str)
assert {(e, f) for e in _reached("gemm") for f in FORMATS} == GEMM_TUPLES
# the run-time epilogue of the direct kernels sees every activation as act and as act2, with a residual
assert all(any(c.act == a and c.res and c.fam == "direct" and dispatch(c)[1] == GEN for c in CASES) and
           any(c.act2 == a and c.res and c.fam == "direct" and dispatch(c)[1] == GEN for c in CASES) for a in ("elu", "prelu", "gelu", "relu"))
# one, two and three or more K chunks (three copies of the main loop) and a ragged last chunk, per kernel family
for _fam, _ks in (("direct", 1), ("direct", 3), ("direct", 7), ("wino", 3), ("wino2d", 3), ("gemm", 1)):
    _sel = [c for c in CASES if c.fam == _fam and c.ks == _ks]
    assert {min(nchunks(c), 3) for c in _sel} == {1, 2, 3}, (_fam, _ks)
    assert any(packed_cin(c) % (CK[_ks] if _fam == "direct" else 8 if _ks == 3 else 16) for c in _sel), (_fam, _ks)
# the pointer-alone cases are scalar-staged / unaligned although W % 4 == 0
assert all(c.W % 4 == 0 for c in CASES if c.mis in ("x", "add"))
assert {dispatch(c)[0] for c in CASES if c.fam == "direct" and c.mis in ("x", "add")} == {"C1_64"}
assert {dispatch(c)[2] for c in CASES if c.fam == "wino2d" and c.mis in ("x", "add")} == {False}
# EPI_UP: with and without aff+add on both 128-channel tilings; out_blocked on the four tilings that build it
assert all((t, U, p) in _reached("direct") for t in ("C1_128", "C1v_128") for p in (False, True))
assert {dispatch(c)[0] for c in CASES if c.blk} == {"C1_64", "C1v_64", "C1_128", "C1v_128"}


# ------------------------------------------------------------------------------------------------ fixtures
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
    with torch.no_grad():
        yield
    ops.set_option("winograd_min_cout", 1)
    ops.set_option("winograd_2d", ops.WINOGRAD_2D_DEFAULT)
    ops.set_precision("fp32")


def set_family_options(ops, c):
    ops.set_option("winograd_min_cout", 1 << 20 if c.fam == "direct" else 1)
    ops.set_option("winograd_2d", 1 if c.fam == "wino2d" else ops.WINOGRAD_2D_DEFAULT)


# ------------------------------------------------------------------------------------------------ inputs and references
_INPUTS, _LIN = {}, {}


def oshape(c, B=None):
    B = c.B if B is None else B
    return (B, c.cout // 4, 2 * c.H, 2 * c.W) if c.up else (B, c.cout, c.H, c.W)


def inputs(c):
    """Seeded CPU tensors of a case; with a load-side prologue x, sc, sh and add lie on the dyadic grid of
    test_gpu_split_dispatch.inputs (x * sc + sh + add is exact in fp32, fused or rounded twice).  Two-source inputs: "x" holds the
    concatenation, w the unpadded bank."""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    B = c.B

    def dy(*s):
        return torch.randint(-127, 128, s, generator=g).float() / 16

    t = {"x": dy(B, c.cin, c.H, c.W) if c.pro else torch.randn(B, c.cin, c.H, c.W, generator=g)}
    if c.up:                                                   # ConvTranspose2d weight [Cin, Co, 2, 2], bias [Co]
        t["w"] = torch.randn(c.cin, c.cout // 4, 2, 2, generator=g) / c.cin ** 0.5
        t["b"] = torch.randn(c.cout // 4, generator=g)
    else:
        t["w"] = torch.randn(c.cout, c.cin, c.ks, c.ks, generator=g) / (c.cin * c.ks * c.ks) ** 0.5
        t["b"] = torch.randn(c.cout, generator=g)
    if c.res:
        t["res"] = torch.randn(oshape(c), generator=g)
    if "prelu" in (c.act, c.act2):
        t["alpha"] = torch.tensor([0.2])
    if "aff" in c.pro:
        shp = (c.cin,) if "aff1" in c.pro else (B, c.cin)
        t["sc"] = 2.0 ** torch.randint(-1, 2, shp, generator=g).float()
        t["sh"] = dy(*shp)
    if "add" in c.pro:
        t["add"] = dy(B, c.cin, c.H, c.W)
    _INPUTS[c.name] = t
    return t


def linear(c, rnd):
    """float64 convolution (no bias) of the operands rounded by rnd (None: exact), once per (case, rounding)"""
    key = (c.name, None if rnd is None else rnd.__name__)
    if key not in _LIN:
        t = inputs(c)
        r = rnd or (lambda v: v.double())
        xin = _pro32(t["x"], t.get("sc"), t.get("sh"), t.get("add"))       # fp32, exact (dyadic grid)
        _LIN[key] = F.conv_transpose2d(r(xin), r(t["w"]), stride=2) if c.up else F.conv2d(r(xin), r(t["w"]), padding=c.ks // 2)
    return _LIN[key]


def _act(v, a, alpha):
    if a is None:
        return v
    if a == "prelu":
        return torch.where(v > 0, v, float(alpha) * v)
    return {"elu": F.elu, "gelu": F.gelu, "relu": F.relu}[a](v)


def reference(c, rnd=None):
    t = inputs(c)
    v = _act(linear(c, rnd) + t["b"].double().view(1, -1, 1, 1), c.act, t.get("alpha"))
    if c.res:
        v = v + t["res"].double()
    return _act(v, c.act2, t.get("alpha"))


def check(c, fmt, got, what=""):
    """the bound of the kernel family / operand format (see the module docstring); prints the figure before it asserts"""
    if fmt in ("bf16", "fp16"):
        own, other = (b16, h) if fmt == "bf16" else (h, b16)
        ref, ref_other = reference(c, own), reference(c, other)
        print(f"maxrel {c.fam} {fmt} {c.name} {what}: {maxrel(got, ref):.3e} (other format {maxrel(got, ref_other):.3e}), bound {F16_TOL:g}")
        check16(got, ref, ref_other, f"{c.name} {fmt} {what}")
        return
    plain = c.act is None and c.act2 is None and not c.res
    tol = SPLIT_TOL if c.fam == "gemm" else WINO_TOL if c.fam in ("wino", "wino2d") else DIRECT_TOL if plain else DIRECT_EPI_TOL
    print(f"maxrel {c.fam} {fmt} {c.name} {what}: {rel_err(got, reference(c))[0]:.3e}, bound {tol:g}")
    assert_close(got, reference(c), tol, f"{c.name} {fmt} {what}")


# ------------------------------------------------------------------------------------------------ device layouts and launches
def nan_around(shape, before, after, off=0):
    """a [B,C,H,W] view that is the channel slice [before, before + C) of a NaN-filled [B, before + C + after, H, W] tensor starting
    ``off`` floats into its (aligned) allocation; -> (view, whole allocation)"""
    B, Cc, H, W = shape
    n = B * (before + Cc + after) * H * W
    flat = torch.full((n + 4,), NAN, device="cuda")
    return flat[off:off + n].view(B, before + Cc + after, H, W)[:, before:before + Cc], flat


def sliced(t, before, after, off=0):
    v, flat = nan_around(tuple(t.shape), before, after, off)
    v.copy_(t)
    return v


def untouched_outside(view, flat):
    """every element of the allocation outside the view still has the NaN bit pattern it was filled with"""
    probe = flat.clone()
    probe.as_strided(view.size(), view.stride(), view.storage_offset() - flat.storage_offset()).fill_(NAN)
    return bool((probe.view(torch.int32) == NAN_BITS).all())


def _to_dev(t, key):
    return t[key].cuda() if key in t else None


class Dev:
    """the case's tensors on the device in the layouts the launches read: x, the skip tensor, the residual and both sources of a
    two-source input as channel slices between NaN channels (batch strides above their channel counts)"""

    def __init__(self, c):
        t = inputs(c)
        self.c = c
        if c.cat:
            self.x = sliced(t["x"][:, :c.cat], 2, 3)
            self.x2 = sliced(t["x"][:, c.cat:], 1, 3)
        else:
            self.x, self.x2 = sliced(t["x"], 2, 3, off=int(c.mis == "x")), None
        self.w, self.b = t["w"].cuda(), t["b"].cuda()
        self.alpha, self.sc, self.sh = _to_dev(t, "alpha"), _to_dev(t, "sc"), _to_dev(t, "sh")
        self.res = sliced(t["res"], 1, 2) if c.res else None
        self.add = sliced(t["add"], 1, 3, off=int(c.mis == "add")) if "add" in t else None

    def pack(self, ops):
        c = self.c
        self.pc = ops.pack_conv_weight_cat(self.w, c.cat) if c.cat else ops.pack_conv_weight(self.w, transposed=c.up)
        assert self.pc.split == (c.fam == "gemm") and self.pc.ks == c.ks and self.pc.cout == c.cout
        return self

    def rows16(self):
        """the alignment predicate of the host code on the tensors as they are"""
        c = self.c
        ts = [self.x] + ([self.add] if self.add is not None else [])
        return c.W % 4 == 0 and all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 for t in ts)

    def out(self, B=None):
        """the output as a channel slice of a NaN-filled tensor (blocked: 16-byte aligned, as the entry point requires) -> (view, allocation)"""
        c = self.c
        return nan_around(oshape(c, B), 4, 4) if c.blk else nan_around(oshape(c, B), 3, 2, off=int(c.mis == "y"))

    def run(self, ops, s=None, out=None, blk=None):
        """one launch over the whole batch, or (s = sample index) over sample s alone"""
        c = self.c
        sl = slice(None) if s is None else slice(s, s + 1)

        def per(t):
            return None if t is None else t[sl]
        sc = self.sc if self.sc is None or self.sc.dim() == 1 else self.sc[sl]
        sh = self.sh if self.sh is None or self.sh.dim() == 1 else self.sh[sl]
        return ops.conv2d(self.x[sl], self.pc, bias=self.b, act=c.act, prelu_alpha=self.alpha, residual=per(self.res), act2=c.act2,
                          in_scale=sc, in_shift=sh, in_add=per(self.add), out=out, cat=per(self.x2),
                          out_blocked=c.blk if blk is None else blk)


def _from_blocked(t):
    B, Cc, H, W = t.shape
    return t.reshape(B, Cc // 8, H, W, 8).permute(0, 1, 4, 2, 3).contiguous().view(B, Cc, H, W)


def launch_and_check(ops, c, fmt):
    """the float64 bound, no store outside the output, no leak from the NaN neighbours (a leak is a NaN in the output), batch"""
    d = Dev(c).pack(ops)
    assert d.rows16() == rows16(c), (c.name, "the layout does not give the alignment the case stands for")
    out, flat = d.out()
    assert not c.up or (out.data_ptr() % 8 != 0) == (c.mis == "y")       # (EPI_UP: 8-byte stores or their fallback)
    y = d.run(ops, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    assert untouched_outside(out, flat), (c.name, fmt, "a store outside the output slice")
    check(c, fmt, _from_blocked(y) if c.blk else y)
    if c.blk:                                                 # the same arithmetic as the NCHW launch, only the memory order differs
        assert torch.equal(_from_blocked(y), d.run(ops, blk=False)), (c.name, "out_blocked vs NCHW")
    for s in range(c.B):
        assert torch.equal(d.run(ops, s=s), y[s:s + 1]), (c.name, fmt, "sample", s)
    return d


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("c", FP32_CASES, ids=[c.name for c in FP32_CASES])
def test_fp32_kernel_launch_vs_float64(c):
    """one instantiation of the direct / Winograd kernels"""
    from cwfa_amd import ops
    ops.set_precision("fp32")
    set_family_options(ops, c)
    launch_and_check(ops, c, "fp32")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("c", GEMM_CASES, ids=[c.name for c in GEMM_CASES])
def test_split_gemm_launch_vs_float64(c, fmt, monkeypatch):
    """one epilogue of the split 1x1 GEMM in one operand format; the prologue is applied by cwfa_split_input_f32, not by the GEMM"""
    from cwfa_amd import _lib, ops
    ops.set_precision(fmt)
    L = _lib.lib()
    calls = []
    split_input, gemm = L.cwfa_split_input_f32, L.cwfa_conv_split_f32

    def rec_input(*a):
        calls.append(("input", a[6] is not None, a[7] is not None, a[9] is not None))
        return split_input(*a)

    def rec_gemm(*a):
        o = a[10]._obj
        calls.append(("gemm", bool(o.in_scale), bool(o.in_shift), bool(o.in_add)))
        return gemm(*a)
    monkeypatch.setattr(L, "cwfa_split_input_f32", rec_input)
    monkeypatch.setattr(L, "cwfa_conv_split_f32", rec_gemm)
    launch_and_check(ops, c, fmt)
    aff, add = "aff" in c.pro, "add" in c.pro
    assert calls and calls == [("input", aff, aff, add), ("gemm", False, False, False)] * (len(calls) // 2), (c.name, fmt, calls)


@pytest.mark.parametrize("shape", [(1, 16, 32), (2, 19, 45), (1, 5, 7)])
def test_subnet_layer_tape_fp32_vs_float64(shape):
    """cwfa_subnet_layer_tape_f32 (wino_layer_kernel<true>): y and the hidden map ELU(conv3x3(x) + b3) against float64, y bit-equal
    to the launch without the tape, x a channel slice between NaN channels"""
    from cwfa_amd import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(H * W + 3)
    x = torch.randn(B, 64, H, W, generator=g)
    w3, b3 = torch.randn(64, 64, 3, 3, generator=g) / 24, torch.randn(64, generator=g) * 0.1
    w1, b1 = torch.randn(64, 64, 1, 1, generator=g) / 8, torch.randn(64, generator=g) * 0.1
    href = F.elu(F.conv2d(x.double(), w3.double(), b3.double(), padding=1))
    ref = F.elu(F.conv2d(href, w1.double(), b1.double()) + x.double())
    xs = sliced(x, 2, 3)
    pc3, panel = ops.pack_conv_weight(w3.cuda()), ops.pack_1x1_panel(w1.cuda())
    assert not pc3.split
    y0 = ops.subnet_layer(xs, pc3, b3.cuda(), panel, b1.cuda())
    y, hid = ops.subnet_layer(xs, pc3, b3.cuda(), panel, b1.cuda(), want_hidden=True)
    print(f"maxrel layer fp32 {shape}: y {rel_err(y, ref)[0]:.3e}, hidden {rel_err(hid, href)[0]:.3e}, bound 3e-06")
    assert torch.equal(y, y0), "y with and without the tape"
    assert_close(y, ref, 3e-6, "y of the tape form")
    assert_close(hid, href, 3e-6, "hidden map of the tape form")


def _all_nan(t):
    torch.cuda.synchronize()
    return bool((t.view(torch.int32) == NAN_BITS).all())


def test_empty_and_rejected_calls_launch_nothing():
    """the argument checks of the fp32 entry points: an empty problem returns CWFA_OK, a rejected one its error code, and neither
    touches the output"""
    from cwfa_amd import _lib, ops
    from cwfa_amd._lib import ConvOpts
    L = _lib.lib()
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 8, 32
    x = torch.randn(B, 23, H, W, generator=g).cuda()
    y = torch.full((B, 72, H, W), NAN, device="cuda")
    bias = torch.randn(72, generator=g).cuda()

    def raw(pc, cin, cout, o, B=B, H=H):
        return L.cwfa_conv2d_f32(ops._p(x), ops._p(pc.packed), ops._p(y), B, cin, H, W, cout, pc.ks, 23 * H * W, 72 * H * W, C.byref(o),
                                 ops._stream())

    pc1 = ops.pack_conv_weight(torch.randn(64, 16, 1, 1, generator=g).cuda())
    pc3 = ops.pack_conv_weight(torch.randn(64, 16, 3, 3, generator=g).cuda())           # (Winograd image)
    for pc in (pc1, pc3):
        o = ConvOpts()
        o.bias = bias.data_ptr()
        assert raw(pc, 16, 64, o, B=0) == 0 and raw(pc, 16, 64, o, H=0) == 0
    assert tuple(ops.conv2d(x[:0, :16], pc1, bias=bias[:64]).shape) == (0, 64, H, W)
    assert tuple(ops.conv2d(x[:, :16, :0], pc3, bias=bias[:64]).shape) == (B, 64, 0, W)
    panel = ops.pack_1x1_panel(torch.randn(64, 64, 1, 1, generator=g).cuda())
    pl = ops.pack_conv_weight(torch.randn(64, 64, 3, 3, generator=g).cuda())
    hid = torch.full((B, 64, H, W), NAN, device="cuda")
    x64 = torch.randn(B, 64, H, W, generator=g).cuda()
    for b_, h_ in ((0, H), (B, 0)):
        assert L.cwfa_subnet_layer_tape_f32(ops._p(x64), ops._p(pl.packed), ops._p(bias), ops._p(panel.packed), ops._p(bias), ops._p(y),
                                            ops._p(hid), b_, h_, W, 64 * H * W, 72 * H * W, 64 * H * W, ops._stream()) == 0
    assert _all_nan(y) and _all_nan(hid), "an empty problem wrote its output"
    # out_blocked with a load-side prologue: CWFA_E_INVAL
    sc = torch.ones(16, device="cuda")
    with pytest.raises(_lib.CwfaHipError, match=r"code -1\)"):
        ops.conv2d(x[:, :16], pc1, bias=bias[:64], in_scale=sc, in_shift=sc, out=y[:, :64], out_blocked=True)
    assert _all_nan(y)
    # out_blocked on a bank with <= 32 outputs (no such instantiation): CWFA_E_SHAPE
    pc32 = ops.pack_conv_weight(torch.randn(32, 16, 1, 1, generator=g).cuda())
    o = ConvOpts()
    o.bias, o.out_blocked8 = bias.data_ptr(), 1
    assert raw(pc32, 16, 32, o) == -2
    with pytest.raises(ValueError):
        ops.conv2d(x[:, :16], pc32, bias=bias[:32], out_blocked=True)
    assert _all_nan(y)
    # a two-source input into a bank with more than 64 outputs: CWFA_E_INVAL
    pc72 = ops.pack_conv_weight(torch.randn(72, 23, 1, 1, generator=g).cuda())
    o = ConvOpts()
    o.bias, o.in_cat, o.in_cat_bs, o.in_cat_from, o.in_cat_c1 = bias.data_ptr(), x.data_ptr(), 23 * H * W, 16, 5
    assert raw(pc72, 23, 72, o) == -1
    o.in_cat = None
    assert raw(pc72, 23, 72, o) == 0                          # (the same call without the second source is accepted)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y).any())


if __name__ == "__main__":                                    # CPU only: the float64 references of every case build
    import time
    t0 = time.time()
    for c_ in CASES:
        for rnd_ in (None,) if c_.fam != "gemm" else (None, b16, h):
            r_ = reference(c_, rnd_)
            assert tuple(r_.shape) == oshape(c_) and bool(torch.isfinite(r_).all()), c_.name
    print(f"{len(CASES)} cases ({len(FP32_CASES)} fp32 + {len(GEMM_CASES)} GEMM x 3 formats): "
          f"{len(_LIN)} float64 references in {time.time() - t0:.1f} s")
