"""GPU (MI355X): every launch form of the convolution weight gradients and of the Conv3d stage's backward (csrc/conv_bwd.hip)
against float64 -- bit for bit on integer data, and within rounding bounds on random data.

Routes of cwfa_conv2d_wgrad_f32 (`dispatch` restates the host selection, `geom` its launch geometry):
  k1, k3, k7      conv_wgrad_kernel<1,1> / <3,3> / <1,7> (seven row passes): register-staged strips, double-buffered
  rows            conv_wgrad_rows_kernel: the 3x3 form for 16-byte aligned rows (LDS-DMA, `issue(next, buf ^ 1)`)
  split3x3_six / split3x3_one / split1x1_six / split1x1_one
                  conv_wgrad_split_kernel<SIX, KS>: the bf16 matrix-core walk over units of SEG = 32 rows, in the split
                  arithmetic ("split_bf16") or with plain bf16 operands ("bf16" and "fp16" precision)
  empty           B, H or W zero: the reduction kernel alone (dw = beta * dw)
Kernels of the four cwfa_conv3d_* entry points: conv3d_hidden_fwd_kernel / conv3d_hidden4_kernel<+1>, conv3d_hidden_bwd_kernel /
conv3d_hidden4_kernel<-1>, conv3d_input_bwd_kernel / conv3d_input_bwd4_kernel, conv3d_wgrad_kernel / conv3d_wgrad4_kernel (the
four-voxel forms run for W % 4 == 0 from 16-byte aligned buffers, the scalar forms otherwise).

Regimes, asserted at import for the case lists: every 2-D route and both 3-D weight-gradient kernels have a case with one strip
(unit, item) per worker (block, wave) and a case where some workers walk at least two and others fewer (a ragged division: the
`more` branch, stash(buf ^ 1) and the buffer flip; issue(next, buf ^ 1); the split form's unit loop with its leading barrier); the
split forms have cases with several units per block across a SEG border, one with a last segment of a single row (H = 33), and
one-tile cases with more than 256 units; the per-voxel 3-D kernels have one-block and ragged several-block cases.  The ineligible
split-mode routes (ks 7, a 1x1 bank above 64 x 64, a misaligned pointer, W % 4 != 0) are in the list and must be bit-equal to
the fp32 mode.  Edges: H = 1, odd H, W < 32, W = 4, W % 32 in {1, 31}, channel counts off the 32 / 64 tiles, Cin = 1,
Cout = 1, B = 3.

The restated worker / block counts are cross-checked against the library inside every weight-gradient test, through
cwfa_conv2d_wgrad_workspace_bytes and cwfa_conv3d_wgrad_workspace_bytes (both encode the count): a change of the host rule
that moves a case off its regime fails the test.  The ONE restated rule without such a query is the split form's grid,
min(workers, ceil(256 / tiles), units): it is restated from the source alone.

Exact tests.  x and dy are integers in -2 .. 2 (exact in fp32, bf16 and fp16; one non-zero piece in the split arithmetic), so
every product is an integer and -- asserted on the host before any launch: pixels * 4 + the accumulation base < 2**24 --
every partial sum in any order is an exact fp32 number: the result must be torch.equal to the float64 reference, for dW and db,
with and without `accumulate` into an integer buffer, on every route.  A dropped, doubled or shifted pixel, row, strip or
worker moves an entry by at least 1.  Every case also runs with x AND dy as channel slices of NaN-filled tensors (batch strides
above the channel counts; the misaligned cases one float past a 16-byte boundary), which must be untouched outside the slices.
The Conv3d entry points run the same way on integer x, dy, w1, b1, w2 and alpha = 0.25 (everything on the grid of 0.25): q, m,
dalpha, dx and both 32 x 32 blocks bit for bit, rows >= K and columns >= 28 zero (beta = 0) or as they were (beta = 1); m and
dalpha come from float64 autograd of F.prelu, so the tie q == 0 (frequent on integer data) follows torch's convention.

Regimes per route, as (workers or blocks, strips or units) of `geom`:
  k3      one (3, 3), (12, 12) ...; ragged (29, 36) at 130 -> 130, (256, 297) on one tile
  rows    one (12, 12), (3, 3) ...; ragged (29, 36), (256, 297)
  k1      one (3, 3) ...; ragged (86, 105) at 130 -> 70, (512, 528) on one tile
  k7      one (3, 3) ...; ragged (43, 60) at 70 -> 130, (256, 272) on one tile -- each of the seven passes
  split3x3_six / _one   one (1, 1), (6, 6); ragged (29, 32) with four row segments per image, (29, 30) with H = 33, (256, 260) on one tile
  split1x1_six / _one   one (1, 1), (12, 12), (6, 6); ragged (256, 300) on one tile with ten row segments per image
  conv3d_wgrad_kernel / conv3d_wgrad4_kernel   at most one item per wave (1 .. 24 items); ragged 2160 items on 2048 waves
With the four loops cut short on purpose (the last strip never loaded in conv_wgrad_kernel and conv_wgrad_rows_kernel, the split
form's second round of units and the Conv3d waves' second items dropped) the weight-gradient and Conv3d tests of
test_gpu_backward.py still pass; here exactly the 18 ragged cases fail.

Rounding tests (random normal data, every figure printed next to its bound with pytest -s).  Largest figures measured on an MI355X:
  fp32 forms      dW: k1 2.0e-7, k3 2.1e-7, k7 1.9e-7, rows 2.0e-7 (bound 5e-6); db 3.5e-7 (5e-6)
  split, six      dW: 3x3 6.6e-7, 1x1 9.2e-7 (bound 3e-6; both on the one-tile cases with > 256 units); db 4.2e-7 (3e-6)
  split, one      dW against bf16-rounded operands: 3x3 2.3e-7, 1x1 2.2e-7 (3e-6); the unrounded reference >= 1.4e-3 away; db 5.1e-7 (3e-6)
  Conv3d          q 2.0e-7, m 2.2e-7, dx 3.1e-7 scalar / 1.9e-7 four-voxel (bound 1e-6)
                  dalpha 0.031 of its per-entry bound (k = 27 + 1 + K + 1), the 32 x 32 blocks 0.021 of theirs (k from the
                  accumulation depth, 70 .. 261)
Finding: before this file, both input-gradient kernels ran ONE fp32 chain through all 27 K terms of a dx element; at K = 32 (864
roundings) dx was 1.03e-6 (scalar) and 9.8e-7 (four-voxel) of its maximum away from float64 on the 9 x 240 x 4 volume -- at and over
the 1e-6 bound.  conv3d_input_bwd_kernel and conv3d_input_bwd4_kernel now keep a running sum per hidden channel (27 + K
roundings); the figures above are with that change.  No other kernel was changed: every exact case passed as the kernels stood.
"""
import ctypes as C
import dataclasses
import zlib
from contextlib import contextmanager
from dataclasses import dataclass

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, rel_err
from split_ref import b16, check16, maxrel
from test_gpu_conv_dispatch import nan_around, sliced, untouched_outside

pytestmark = pytest.mark.gpu
NAN = float("nan")
U = 2.0 ** -24                # unit roundoff of fp32
FP32_TOL = 5e-6               # k1, k3, k7, rows: the bound tools/stress_round3.py holds conv2d_wgrad to
SPLIT_TOL = 3e-6              # the split forms (test_gpu_backward.py); single-product forms against bf16-rounded operands
EW = 1e-6                     # elementwise Conv3d outputs q, m, dx (EW of test_gpu_backward_kernels.py)
SEG = 32                      # ws::SEG, rows per unit of the split form
E_INVAL, E_SHAPE = -1, -2     # CWFA_E_INVAL, CWFA_E_SHAPE (include/cwfa_hip.h)
EXACT_LIMIT = 2 ** 24


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ 2-D: the host selection, restated
@dataclass(frozen=True)
class Case:
    name: str
    ks: int
    B: int
    cin: int
    cout: int
    H: int
    W: int
    mode: str = "fp32"        # ops.set_precision: "fp32" | "split_bf16" | "bf16" | "fp16" (the last three set wgrad_split = 1)
    rows: int = 1             # option "wgrad_rows"
    mis: bool = False         # x and dy start one float past a 16-byte boundary


ROUTES = ("k1", "k3", "k7", "rows", "split3x3_six", "split3x3_one", "split1x1_six", "split1x1_one", "empty")


def rows16(c):
    """W % 4 == 0, 16-byte aligned x and dy.  The other terms of the host predicate follow: H * W and both batch strides (a
    channel count times H * W in the layouts of `operands`) are multiples of four whenever W is."""
    return c.W % 4 == 0 and not c.mis


def dispatch(c):
    """the route cwfa_conv2d_wgrad_f32 takes (conv_bwd.hip, from `if (B == 0 || ...)` down to the last launch)"""
    if c.B == 0 or c.H == 0 or c.W == 0:
        return "empty"
    if c.ks == 7:
        return "k7"
    if (c.ks == 3 or (c.cout <= 64 and c.cin <= 64)) and c.mode != "fp32" and rows16(c):
        return f"split{c.ks}x{c.ks}_" + ("six" if c.mode == "split_bf16" else "one")
    if c.ks == 3:
        return "rows" if c.rows and rows16(c) else "k3"
    return "k1"


def tiles(c):
    return cdiv(c.cout, 64) * cdiv(c.cin, 64)


def workers(c):
    """wgrad_workers (the 7x7 passes take the 3x3 rule)"""
    strips = c.B * cdiv(c.H, 2) * cdiv(c.W, 32)
    return max(1, min(cdiv(512 if c.ks == 1 else 256, tiles(c)), strips))


def geom(c):
    """(workers, strips of 2 rows x 32 pixels) of the fp32 forms; (blocks, units of SEG rows x 32 pixels) of the split form"""
    if dispatch(c).startswith("split"):
        units = c.B * cdiv(c.H, SEG) * cdiv(c.W, 32)
        return min(workers(c), max(1, cdiv(256, tiles(c))), units), units
    return workers(c), c.B * cdiv(c.H, 2) * cdiv(c.W, 32)


def regime(c):
    n, s = geom(c)
    assert 1 <= n <= s
    return "one" if s == n else "ragged" if s % n else "even"


def workspace_bytes(c):
    """cwfa_conv2d_wgrad_workspace_bytes, from the restated worker count"""
    if c.ks == 7:
        return (workers(c) * (c.cout * c.cin * 7 + c.cout) + c.cout * c.cin * 7) * 4
    return workers(c) * (c.cout * c.cin * c.ks * c.ks + c.cout) * 4


def _split(name, ks, B, cin, cout, H, W):
    return [Case(f"{name}_six", ks, B, cin, cout, H, W, mode="split_bf16"), Case(f"{name}_one", ks, B, cin, cout, H, W, mode="bf16")]


CASES = [
    # ---- conv_wgrad_kernel<3,3>: W % 4 != 0, or "wgrad_rows" off, or a misaligned pointer
    Case("k3_1x1ch_h1", 3, 3, 1, 1, 1, 31),                    # Cin = Cout = 1, H = 1, W < 32, B = 3: 3 strips on 3 workers
    Case("k3_ragged", 3, 2, 130, 130, 12, 70),                 # 9 tiles, 29 workers, 36 strips
    Case("k3_tile1_ragged", 3, 1, 64, 64, 65, 258),            # one tile, 256 workers, 297 strips; odd H
    Case("k3_mis", 3, 2, 33, 70, 5, 36, mis=True),             # aligned rows, misaligned pointers: falls from the rows form
    Case("k3_rows_off", 3, 1, 40, 24, 4, 4, rows=0),           # W = 4
    Case("k3_w33", 3, 1, 20, 65, 7, 33),                       # W % 32 == 1
    # ---- conv_wgrad_rows_kernel
    Case("rows_one", 3, 2, 33, 70, 5, 36),
    Case("rows_ragged", 3, 2, 130, 130, 12, 72),               # 29 workers, 36 strips
    Case("rows_tile1_ragged", 3, 1, 64, 64, 66, 260),          # 256 workers, 297 strips
    Case("rows_w4_h1", 3, 3, 5, 3, 1, 4),
    Case("rows_cin1", 3, 1, 1, 64, 9, 100),
    # ---- conv_wgrad_kernel<1,1>
    Case("k1_1x1ch_h1", 1, 3, 1, 1, 1, 31),
    Case("k1_ragged", 1, 1, 130, 70, 14, 479),                 # 6 tiles, 86 workers, 105 strips; W % 32 == 31
    Case("k1_tile1_ragged", 1, 1, 64, 64, 66, 500),            # one tile, 512 workers, 528 strips
    Case("k1_w32", 1, 2, 17, 33, 8, 32),
    Case("k1_w4", 1, 3, 9, 1, 3, 4),                           # Cout = 1
    # ---- conv_wgrad_kernel<1,7>, seven passes
    Case("k7_one", 7, 1, 3, 7, 5, 20),
    Case("k7_ragged", 7, 1, 70, 130, 11, 300),                 # 6 tiles, 43 workers, 60 strips
    Case("k7_tile1_ragged", 7, 1, 8, 8, 33, 500),              # 256 workers, 272 strips
    Case("k7_b3_w33", 7, 3, 1, 5, 1, 33),
    # ---- conv_wgrad_split_kernel<SIX, 3>
    *_split("s3_one", 3, 1, 8, 8, 6, 4),
    *_split("s3_ragged", 3, 2, 130, 130, 100, 128),            # 29 blocks, 32 units, four row segments per image
    *_split("s3_h33_ragged", 3, 3, 130, 130, 33, 160),         # 29 blocks, 30 units; the last segment has one row
    *_split("s3_tile1_ragged", 3, 2, 16, 16, 130, 832),        # one tile, 256 blocks, 260 units
    *_split("s3_odd", 3, 3, 29, 48, 16, 36),
    # ---- conv_wgrad_split_kernel<SIX, 1>
    *_split("s1_one", 1, 1, 8, 8, 6, 4),
    *_split("s1_tile1_ragged", 1, 3, 24, 40, 320, 320),        # 256 blocks, 300 units
    *_split("s1_odd", 1, 3, 29, 48, 33, 36),
    *_split("s1_cout1", 1, 2, 64, 1, 70, 8),
    # ---- split mode, not eligible: must run (and be bit-equal to) the fp32 route
    Case("inel_k7", 7, 2, 9, 12, 6, 36, mode="split_bf16"),
    Case("inel_k1_bank", 1, 2, 65, 64, 6, 36, mode="split_bf16"),
    Case("inel_k1_bank_bf16", 1, 1, 16, 70, 5, 8, mode="bf16"),
    Case("inel_k3_mis", 3, 2, 20, 24, 6, 36, mode="split_bf16", mis=True),
    Case("inel_k3_mis_bf16", 3, 1, 64, 64, 34, 32, mode="bf16", mis=True),
    Case("inel_k3_w", 3, 2, 20, 24, 6, 35, mode="split_bf16"),
]
INELIGIBLE = [c for c in CASES if c.name.startswith("inel_")]
ONE_FORMS = [c for c in CASES if dispatch(c).endswith("_one")]
EMPTY_CASES = [Case("empty_b0", 3, 0, 5, 3, 4, 4), Case("empty_h0", 1, 2, 5, 3, 0, 4), Case("empty_w0", 7, 2, 3, 2, 4, 0)]

# ---- reach (at import: no GPU needed)
assert len({c.name for c in CASES}) == len(CASES)
_by_route = {r: [c for c in CASES if dispatch(c) == r] for r in ROUTES}
assert {dispatch(c) for c in EMPTY_CASES} == {"empty"} and not _by_route["empty"]
for _r in ROUTES[:-1]:
    assert {"one", "ragged"} <= {regime(c) for c in _by_route[_r]}, (_r, [(c.name, geom(c)) for c in _by_route[_r]])
    if _r.startswith("split"):
        assert any(regime(c) == "ragged" and c.H > SEG for c in _by_route[_r]), _r          # several units per block across a SEG border
        assert any(geom(c)[1] > 256 and tiles(c) == 1 for c in _by_route[_r]), _r             # one tile: the 256-block cap
assert any(c.H == 33 and regime(c) == "ragged" for c in _by_route["split3x3_six"] + _by_route["split3x3_one"])
# the geometry the case names promise
_g = {c.name: geom(c) for c in CASES}
assert (_g["k3_ragged"], _g["rows_ragged"], _g["k3_tile1_ragged"], _g["rows_tile1_ragged"]) == ((29, 36), (29, 36), (256, 297), (256, 297))
assert (_g["k1_ragged"], _g["k1_tile1_ragged"], _g["k7_ragged"], _g["k7_tile1_ragged"]) == ((86, 105), (512, 528), (43, 60), (256, 272))
assert (_g["s3_ragged_six"], _g["s3_h33_ragged_one"], _g["s3_tile1_ragged_six"], _g["s1_tile1_ragged_one"]) == ((29, 32), (29, 30), (256, 260), (256, 300))
# the ineligible split-mode routes: ks 7, a 1x1 bank above 64 x 64 (either side), a misaligned pointer, W % 4 != 0
assert all(c.mode != "fp32" for c in INELIGIBLE) and {dispatch(c) for c in INELIGIBLE} == {"k7", "k1", "k3"}
assert {c.mode for c in INELIGIBLE if dispatch(c) == "k1"} == {"split_bf16", "bf16"}
assert any(c.mis for c in INELIGIBLE) and any(c.W % 4 for c in INELIGIBLE if c.ks == 3)
# aligned-row fallbacks of the fp32 3x3 forms: W % 4 == 0 and still conv_wgrad_kernel<3,3>
assert any(c.mis and c.W % 4 == 0 and c.mode == "fp32" for c in _by_route["k3"]) and any(not c.rows for c in _by_route["k3"])
# edges
assert any(c.H == 1 for c in CASES) and any(c.H % 2 and c.H > 1 for c in CASES) and any(c.W < 32 for c in CASES)
assert any(c.W == 4 for c in CASES) and {1, 31} <= {c.W % 32 for c in CASES} and any(c.B == 3 for c in CASES)
assert any(c.cin == 1 for c in CASES) and any(c.cout == 1 for c in CASES)
assert any(c.cin % 32 and c.cout % 32 and c.cin > 64 and c.cout > 64 for c in CASES)
for _r in ROUTES[:-1]:
    assert any(c.cin % 32 or c.cout % 32 for c in _by_route[_r]), _r


# ------------------------------------------------------------------------------------------------ 3-D: forms and geometry, restated
@dataclass(frozen=True)
class C3:
    name: str
    B: int
    D: int
    H: int
    W: int
    K: int
    mis: bool = False         # every volume starts one float past a 16-byte boundary: the scalar kernels run


KERNELS_3D = {("hidden_fwd", False): "conv3d_hidden_fwd_kernel", ("hidden_fwd", True): "conv3d_hidden4_kernel<+1>",
              ("hidden_bwd", False): "conv3d_hidden_bwd_kernel", ("hidden_bwd", True): "conv3d_hidden4_kernel<-1>",
              ("input_bwd", False): "conv3d_input_bwd_kernel", ("input_bwd", True): "conv3d_input_bwd4_kernel",
              ("wgrad", False): "conv3d_wgrad_kernel", ("wgrad", True): "conv3d_wgrad4_kernel"}


def four(c):
    """the four-voxel form of all four entry points: W % 4 == 0 and 16-byte aligned volumes"""
    return c.W % 4 == 0 and not c.mis


def c3_geom(c):
    """c3_wgrad_blocks: (blocks of four waves, items = runs of 64 voxels along x)"""
    items = c.B * c.D * c.H * cdiv(c.W, 64)
    return max(1, min(cdiv(items, 4), 512)), items


def c3_regime(c):
    blocks, items = c3_geom(c)
    return "one" if items <= 4 * blocks else "ragged" if items % (4 * blocks) else "even"


def c3_voxel_blocks(c):
    """(blocks of 256 threads per sample, threads in the last one) of the per-voxel kernels"""
    n = c.D * c.H * c.W // (4 if four(c) else 1)
    return cdiv(n, 256), n % 256


def _both(name, B, D, H, W, K):
    return [C3(name, B, D, H, W, K), C3(name + "_mis", B, D, H, W, K, mis=True)]


C3_CASES = [
    C3("w1", 1, 1, 1, 1, 1),
    C3("w3", 3, 2, 3, 3, 2),
    *_both("w4", 1, 3, 2, 4, 9),
    *_both("w8", 3, 1, 5, 8, 32),
    *_both("w36", 1, 2, 3, 36, 2),
    *_both("w64", 1, 4, 4, 64, 9),
    *_both("w68", 3, 2, 2, 68, 1),
    C3("w130", 1, 2, 3, 130, 32),
    *_both("items2160", 1, 9, 240, 4, 32),                      # 2160 items on 2048 waves; 9 / 34 blocks of the per-voxel kernels
]
assert {(e, four(c)) for c in C3_CASES for e in ("hidden_fwd", "hidden_bwd", "input_bwd", "wgrad")} == set(KERNELS_3D)
for _f in (False, True):
    assert {"one", "ragged"} <= {c3_regime(c) for c in C3_CASES if four(c) == _f}, _f
    _vb = [c3_voxel_blocks(c) for c in C3_CASES if four(c) == _f]
    assert any(b == 1 for b, _ in _vb) and any(b > 1 and tail for b, tail in _vb), _f
assert {c.W for c in C3_CASES} == {1, 3, 4, 8, 36, 64, 68, 130} and {c.K for c in C3_CASES} == {1, 2, 9, 32}
assert {c.B for c in C3_CASES} == {1, 3} and any(c.D == 1 for c in C3_CASES) and any(c.H == 1 for c in C3_CASES)
assert all(any(m.name == c.name + "_mis" for m in C3_CASES) for c in C3_CASES if c.W % 4 == 0 and not c.mis)
assert c3_geom(C3_CASES[-1]) == (512, 2160)


# ------------------------------------------------------------------------------------------------ fixtures and helpers
@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cwfa_amd import _lib
    _lib.lib()
    yield
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def _id(c):
    return c.name


def _seed(name, salt=0):
    return zlib.crc32(name.encode()) + salt


@contextmanager
def options(ops, c):
    """the precision and the "wgrad_rows" option of case c; library defaults afterwards"""
    try:
        ops.set_precision(c.mode)
        ops.set_option("wgrad_rows", c.rows)
        yield
    finally:
        ops.set_precision("fp32")
        ops.set_option("wgrad_rows", 1)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def exact(got, ref, what):
    """torch.equal(got, ref.float()), with the pattern of the mismatch in the message"""
    want = ref.to(device=got.device, dtype=got.dtype)
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    bad = ~((got == want) | (got.isnan() & want.isnan()))
    n = int(bad.sum())
    print(f"{what}: {n} of {got.numel()} entries differ from the float64 reference (required: 0)")
    if n:
        idx = bad.nonzero()[:12].tolist()
        sample = [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx]
        raise AssertionError(f"{what}: {n} of {got.numel()} entries differ; (index, got, want): {sample}")
    assert torch.equal(got, want), what


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def wgrad_ref(x, dy, ks):
    """float64: dW[o][i][ky][kx] = sum_{b,y,x} dy[b][o][y][x] * x[b][i][y + ky - p][x + kx - p] (zero padding), db[o] = sum dy[b][o];
    one matrix product per tap"""
    p = ks // 2
    xd, dd = x.double(), dy.double()
    B, Ci, H, W = xd.shape
    Co = dd.shape[1]
    xp = F.pad(xd, (p, p, p, p))
    A = dd.permute(1, 0, 2, 3).reshape(Co, -1)
    dW = torch.empty(Co, Ci, ks, ks, dtype=torch.float64, device=x.device)
    for ky in range(ks):
        for kx in range(ks):
            dW[:, :, ky, kx] = A @ xp[:, :, ky:ky + H, kx:kx + W].permute(1, 0, 2, 3).reshape(Ci, -1).t()
    return dW, dd.sum((0, 2, 3))


def ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen, device="cuda").float()


def operands(ops, c, x, dy, slices):
    """x and dy in the layout the launch reads: contiguous, or channel slices 2 / 1 channels into NaN-filled tensors of 5 / 3 more
    channels; one float past a 16-byte boundary for the misaligned cases.  -> (x view, its allocation, dy view, its allocation)"""
    xv, xflat = nan_around(tuple(x.shape), 2 if slices else 0, 3 if slices else 0, int(c.mis))
    dv, dflat = nan_around(tuple(dy.shape), 1 if slices else 0, 2 if slices else 0, int(c.mis))
    xv.copy_(x)
    dv.copy_(dy)
    for v in (xv, dv):
        assert ops.planes(v)[0].data_ptr() == v.data_ptr(), "the wrapper would copy this view"
        if c.W % 4 == 0:
            assert v.data_ptr() % 16 == (4 if c.mis else 0)
        if slices and c.B > 1:
            assert v.stride(0) > v.shape[1] * c.H * c.W
    return xv, xflat, dv, dflat


def check_workspace(ops, c):
    """the restated worker count against the library's (the workspace size encodes it)"""
    got = ops._lib.lib().cwfa_conv2d_wgrad_workspace_bytes(c.B, c.cin, c.H, c.W, c.cout, c.ks)
    assert got == workspace_bytes(c), (c.name, "workers restated", workers(c), "workspace bytes", got, workspace_bytes(c))


# ------------------------------------------------------------------------------------------------ B. 2-D, exact
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_wgrad_exact(c):
    """dW and db of every route bit-equal to float64 on integer data: contiguous and NaN-surrounded strided operands, with db and
    without, plain and accumulated into an integer buffer."""
    from cwfa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(_seed(c.name))
    x, dy = ints((c.B, c.cin, c.H, c.W), -2, 2, g), ints((c.B, c.cout, c.H, c.W), -2, 2, g)
    base_w, base_b = ints((c.cout, c.cin, c.ks, c.ks), -8, 8, g), ints((c.cout,), -8, 8, g)
    # every entry's sum of |term| (terms <= 2 * 2, one per pixel; + the base) stays below 2**24: all partial sums are exact in fp32
    assert c.B * c.H * c.W * 4 + 8 < EXACT_LIMIT
    ref_w, ref_b = wgrad_ref(x, dy, c.ks)
    check_workspace(ops, c)
    with options(ops, c):
        for slices in (False, True):
            tag = f"{c.name} [{dispatch(c)} {geom(c)}{' sliced' if slices else ''}]"
            xv, xflat, dv, dflat = operands(ops, c, x, dy, slices)
            got_w, got_b = ops.conv2d_wgrad(xv, dv, c.ks, want_bias=True)
            only_w = ops.conv2d_wgrad(xv, dv, c.ks)
            acc_w, acc_b = ops.conv2d_wgrad(xv, dv, c.ks, out=base_w.clone(), accumulate=True, bias_out=base_b.clone())
            torch.cuda.synchronize()
            assert untouched_outside(xv, xflat) and untouched_outside(dv, dflat), tag
            exact(got_w, ref_w, f"dW {tag}")
            exact(got_b, ref_b, f"db {tag}")
            exact(only_w, ref_w, f"dW without db {tag}")
            exact(acc_w, ref_w + base_w.double(), f"dW accumulated {tag}")
            exact(acc_b, ref_b + base_b.double(), f"db accumulated {tag}")


@pytest.mark.parametrize("c", INELIGIBLE, ids=_id)
def test_wgrad_split_mode_ineligible_is_the_fp32_route(c):
    """ks 7, a 1x1 bank above 64 x 64, a misaligned pointer or W % 4 != 0 in split / bf16 precision: bit-equal to wgrad_split = 0"""
    from cwfa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(_seed(c.name, 1))
    x, dy = torch.randn(c.B, c.cin, c.H, c.W, generator=g, device="cuda"), torch.randn(c.B, c.cout, c.H, c.W, generator=g, device="cuda")
    assert dispatch(c) == dispatch(dataclasses.replace(c, mode="fp32")) and dispatch(c) in ("k1", "k3", "k7")
    out = []
    with options(ops, c):
        xv, _, dv, _ = operands(ops, c, x, dy, True)
        out.append(ops.conv2d_wgrad(xv, dv, c.ks, want_bias=True))
        ops.set_option("wgrad_split", 0)                      # (`options` restores the defaults)
        out.append(ops.conv2d_wgrad(xv, dv, c.ks, want_bias=True))
    with options(ops, dataclasses.replace(c, mode="fp32")):
        out.append(ops.conv2d_wgrad(xv, dv, c.ks, want_bias=True))
    for other in out[1:]:
        assert same_bits(out[0][0], other[0]) and same_bits(out[0][1], other[1]), c.name
    assert not out[0][0].isnan().any()


@pytest.mark.parametrize("c", ONE_FORMS, ids=_id)
def test_wgrad_fp16_mode_is_the_bf16_form(c):
    """"fp16" precision is documented as plain bf16 operands for the weight gradient: bit-equal to "bf16" on random data"""
    from cwfa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(_seed(c.name, 2))
    x, dy = torch.randn(c.B, c.cin, c.H, c.W, generator=g, device="cuda"), torch.randn(c.B, c.cout, c.H, c.W, generator=g, device="cuda")
    out = []
    for case in (c, dataclasses.replace(c, mode="fp16")):
        assert dispatch(case) == dispatch(c)
        with options(ops, case):
            out.append(ops.conv2d_wgrad(sliced(x, 2, 3), sliced(dy, 1, 2), c.ks, want_bias=True))
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]), c.name
    # and it is the bf16 form that ran, not the fp32 one: 2**-9 operand roundings show
    assert maxrel(out[0][0], wgrad_ref(x, dy, c.ks)[0]) > 1e-5


# ------------------------------------------------------------------------------------------------ D. 2-D, rounding
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_wgrad_rounding(c):
    """random normal data on every route against float64 (strided NaN-surrounded operands): fp32 forms 5e-6, split forms 3e-6, the
    single-product forms 3e-6 against operands rounded to bf16 with the unrounded reference at least 10x further away"""
    from cwfa_amd import ops
    route = dispatch(c)
    g = torch.Generator(device="cuda").manual_seed(_seed(c.name, 3))
    x, dy = torch.randn(c.B, c.cin, c.H, c.W, generator=g, device="cuda"), torch.randn(c.B, c.cout, c.H, c.W, generator=g, device="cuda")
    check_workspace(ops, c)
    with options(ops, c):
        xv, xflat, dv, dflat = operands(ops, c, x, dy, True)
        got_w, got_b = ops.conv2d_wgrad(xv, dv, c.ks, want_bias=True)
        torch.cuda.synchronize()
    assert untouched_outside(xv, xflat) and untouched_outside(dv, dflat)
    ref_w, ref_b = wgrad_ref(x, dy, c.ks)
    tol = SPLIT_TOL if route.startswith("split") else FP32_TOL
    if route.endswith("_one"):
        own_w = wgrad_ref(b16(x), b16(dy), c.ks)[0]
        print(f"{c.name} [{route}]: dW max-rel {rel_err(got_w, own_w)[0]:.3e} vs bf16-rounded operands (bound {tol:g}), "
              f"{maxrel(got_w, ref_w):.3e} vs unrounded; db {rel_err(got_b, ref_b)[0]:.3e} (bound {tol:g})")
        check16(got_w, own_w, ref_w, f"dW {c.name}", tol=tol)
        assert_close(got_w, own_w, tol, f"dW {c.name}")
    else:
        print(f"{c.name} [{route}]: dW max-rel {rel_err(got_w, ref_w)[0]:.3e}, db {rel_err(got_b, ref_b)[0]:.3e} (bound {tol:g})")
        assert_close(got_w, ref_w, tol, f"dW {c.name}")
    # the bias gradient is the fp32 sum of the UNROUNDED dy on every route
    assert_close(got_b, ref_b, tol, f"db {c.name}")


# ------------------------------------------------------------------------------------------------ E. 2-D, empty and rejected calls
def _raw_wgrad(ops, x, dy, dw, db, ws, B, Cin, H, W, Cout, ks, beta):
    return ops._lib.lib().cwfa_conv2d_wgrad_f32(_p(x), _p(dy), _p(dw), _p(db), _p(ws), B, Cin, H, W, Cout, ks, Cin * H * W, Cout * H * W,
                                                beta, ops._stream())


@pytest.mark.parametrize("c", EMPTY_CASES, ids=_id)
def test_wgrad_empty_problem(c):
    """B, H or W zero: beta = 0 writes zeros over NaN, beta = 1 leaves dw and db bit-identical"""
    from cwfa_amd import ops
    assert dispatch(c) == "empty"
    assert ops._lib.lib().cwfa_conv2d_wgrad_workspace_bytes(c.B, c.cin, c.H, c.W, c.cout, c.ks) == 0
    x, dy, ws = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda"), torch.zeros(4096, device="cuda")
    shape = (c.cout, c.cin, c.ks, c.ks)
    dw, db = torch.full(shape, NAN, device="cuda"), torch.full((c.cout,), NAN, device="cuda")
    assert _raw_wgrad(ops, x, dy, dw, db, ws, c.B, c.cin, c.H, c.W, c.cout, c.ks, 0.0) == 0
    assert same_bits(dw, torch.zeros_like(dw)) and same_bits(db, torch.zeros_like(db))
    g = torch.Generator(device="cuda").manual_seed(_seed(c.name))
    w0, b0 = torch.randn(shape, generator=g, device="cuda"), torch.randn(c.cout, generator=g, device="cuda")
    dw, db = w0.clone(), b0.clone()
    assert _raw_wgrad(ops, x, dy, dw, db, ws, c.B, c.cin, c.H, c.W, c.cout, c.ks, 1.0) == 0
    assert same_bits(dw, w0) and same_bits(db, b0)
    dw = torch.full(shape, NAN, device="cuda")
    assert _raw_wgrad(ops, x, dy, dw, None, ws, c.B, c.cin, c.H, c.W, c.cout, c.ks, 0.0) == 0          # db == NULL
    assert same_bits(dw, torch.zeros_like(dw))


def test_wgrad_rejected_calls_touch_nothing():
    """every rejected call returns its code and leaves NaN-filled outputs as they were; all pointers are real allocations at least as
    large as the arguments describe, so a broken check could not read or write out of bounds"""
    from cwfa_amd import ops
    L = ops._lib.lib()
    B, Cin, H, W, Cout = 1, 2, 4, 4, 2
    x, dy = torch.ones(B, Cin, H, W, device="cuda"), torch.ones(B, Cout, H, W, device="cuda")
    ws = torch.zeros(1 << 16, device="cuda")
    dw, db = torch.full((Cout, Cin, 7, 7), NAN, device="cuda"), torch.full((Cout,), NAN, device="cuda")
    calls = [("ks = 5", E_SHAPE, (x, dy, dw, db, ws, B, Cin, H, W, Cout, 5)), ("ks = 2", E_SHAPE, (x, dy, dw, db, ws, B, Cin, H, W, Cout, 2)),
             ("x null", E_INVAL, (None, dy, dw, db, ws, B, Cin, H, W, Cout, 3)), ("dy null", E_INVAL, (x, None, dw, db, ws, B, Cin, H, W, Cout, 3)),
             ("dw null", E_INVAL, (x, dy, None, db, ws, B, Cin, H, W, Cout, 3)), ("workspace null", E_INVAL, (x, dy, dw, db, None, B, Cin, H, W, Cout, 3)),
             ("B < 0", E_SHAPE, (x, dy, dw, db, ws, -1, Cin, H, W, Cout, 3)), ("Cin = 0", E_SHAPE, (x, dy, dw, db, ws, B, 0, H, W, Cout, 3)),
             ("Cout = 0", E_SHAPE, (x, dy, dw, db, ws, B, Cin, H, W, 0, 1)), ("H < 0", E_SHAPE, (x, dy, dw, db, ws, B, Cin, -1, W, Cout, 7))]
    for what, code, args in calls:
        assert _raw_wgrad(ops, *args, 0.0) == code, what
        torch.cuda.synchronize()
        assert dw.isnan().all() and db.isnan().all(), what
        assert L.cwfa_last_error(), what
    # 64 * H * W * 4 == 2**31: one image plane too large for the kernels' 32-bit offsets (a 1 x 1 x 4096 x 2048 pair, 33 MB each)
    H, W = 4096, 2048
    x, dy = torch.ones(1, 1, H, W, device="cuda"), torch.ones(1, 1, H, W, device="cuda")
    ws = torch.zeros(max(L.cwfa_conv2d_wgrad_workspace_bytes(1, 1, H, W, 1, 3), 16) // 4 + 4, device="cuda")
    dw, db = torch.full((1, 1, 3, 3), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    for ks in (1, 3):
        assert _raw_wgrad(ops, x, dy, dw, db, ws, 1, 1, H, W, 1, ks, 0.0) == E_SHAPE
    torch.cuda.synchronize()
    assert dw.isnan().all() and db.isnan().all()


# ------------------------------------------------------------------------------------------------ 3-D references (float64, CPU)
def to_vol(t):
    """[B,D,H,W] / [B,K,D,H,W] (depth as the channel axis) -> torch's [B,C,H,W,D] (networks.py:239)"""
    return t.permute(0, 2, 3, 1).unsqueeze(1) if t.dim() == 4 else t.permute(0, 1, 3, 4, 2)


def from_vol(v):
    """[B,C,H,W,D] -> [B,C,D,H,W], or [B,D,H,W] for C == 1 inputs of `to_vol`"""
    return v.permute(0, 1, 4, 2, 3).contiguous()


def c3_inputs(c, integer):
    g = torch.Generator().manual_seed(_seed(c.name.removesuffix("_mis"), int(integer)))      # (a twin pair shares its data)
    vol = (c.B, c.D, c.H, c.W)
    if integer:
        ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float()      # noqa: E731
        return ri(vol, -2, 2), ri(vol, -2, 2), ri((c.K, 1, 3, 3, 3), -1, 1), ri((c.K,), -1, 1), ri((1, c.K, 3, 3, 3), -1, 1)
    rn = lambda shape, s: torch.randn(shape, generator=g) * s                                # noqa: E731
    return rn(vol, 1.0), rn(vol, 1.0), rn((c.K, 1, 3, 3, 3), 0.3), rn((c.K,), 0.1), rn((1, c.K, 3, 3, 3), 0.3)


def c3_reference(x, dy, w1, b1, w2, alpha):
    """The stage's backward in float64 autograd, cut where the library materialises a volume: the steps after q (after m) start from
    q (m) rounded to fp32, as the kernels read them, so no step inherits the rounding (or a flipped PReLU branch) of the one before."""
    xd = to_vol(x.double()).clone().requires_grad_()
    w1d, b1d = w1.double().requires_grad_(), b1.double().requires_grad_()
    q = F.conv3d(xd, w1d, b1d, padding=1)                                       # [B,K,H,W,D]
    q32 = q.detach().float()
    ql, ad, w2d = q32.double().requires_grad_(), torch.tensor([alpha], dtype=torch.float64, requires_grad=True), w2.double().requires_grad_()
    F.conv3d(F.prelu(ql, ad), w2d, None, padding=1).backward(to_vol(dy.double()))
    m32 = ql.grad.float()
    q.backward(m32.double())
    # |terms| of dalpha = sum_{q <= 0} (W2^T * dy) * q, the factor W2^T * dy counted as the sum of the |w2| * |dy| of its parts
    dh_abs = F.conv_transpose3d(to_vol(dy.double().abs()), w2.double().abs(), padding=1)
    return {"q": from_vol(q.detach()), "q32": from_vol(q32), "m": from_vol(ql.grad), "m32": from_vol(m32), "dalpha": ad.grad,
            "dalpha_abs": (dh_abs * ql.detach().abs() * (ql.detach() <= 0)).sum(), "dx": from_vol(xd.grad)[:, 0],
            "dW2": w2d.grad[0].reshape(-1, 27), "dW1": w1d.grad[:, 0].reshape(-1, 27), "db1": b1d.grad}


def wgrad3d_ref(a, src, alpha, sign, want_bias):
    """the header's contract, restated: out32[k][tap] = sum_p act(a[k][p]) * src[p + sign * (tap - 1)], tap = (ih * 3 + iw) * 3 + id
    over (H, W, depth); column 27 = sum_p act(a[k][p]) if want_bias; everything else 0.  a [B,K,D,H,W], src [B,D,H,W], float64"""
    act = a if alpha is None else torch.where(a > 0, a, alpha * a)
    B, K, D, H, W = a.shape
    sp = F.pad(src, (1, 1, 1, 1, 1, 1))
    out = torch.zeros(32, 32, dtype=torch.float64)
    for t in range(27):
        oy, ox, od = sign * (t // 9 - 1), sign * (t // 3 % 3 - 1), sign * (t % 3 - 1)
        out[:K, t] = torch.einsum("bkdhw,bdhw->k", act, sp[:, 1 + od:1 + od + D, 1 + oy:1 + oy + H, 1 + ox:1 + ox + W])
    if want_bias:
        out[:K, 27] = act.sum((0, 2, 3, 4))
    return out


def dev_buf(t, mis, fill=None):
    """a device copy of t (or, with `fill`, a tensor of t's shape filled with it) inside a NaN-filled allocation, starting
    4 floats (aligned) or 5 floats (one past a 16-byte boundary) in -> (view, allocation)"""
    off = 4 + int(mis)
    flat = torch.full((t.numel() + 12,), NAN, device="cuda")
    v = flat[off:off + t.numel()].view(t.shape)
    if fill is None:
        v.copy_(t)
    else:
        v.fill_(fill)
    assert v.data_ptr() % 16 == (4 if mis else 0)
    return v, flat


def assert_sum_bound(got, ref, absterms, k, what):
    """|got - ref| <= k * 2**-24 * sum |term|, per entry (the bound of test_gpu_backward_kernels.py); prints the largest ratio"""
    got, ref, absterms = (torch.as_tensor(t).double().cpu().reshape(-1) for t in (got, ref, absterms))
    err, bound = (got - ref).abs(), k * U * absterms
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: largest |err| / (k * 2^-24 * sum|term|) = {ratio:.3e} (bound 1, k = {k})")
    assert bool((err <= bound).all()), (what, ratio, k)


# ------------------------------------------------------------------------------------------------ C / D. the Conv3d entry points
ALPHA = 0.25


def run_c3(c, integer):
    from cwfa_amd import ops
    L, st = ops._lib.lib(), ops._stream()
    B, D, H, W, K = c.B, c.D, c.H, c.W, c.K
    dims = (B, D, H, W, K)
    x, dy, w1, b1, w2 = c3_inputs(c, integer)
    R = c3_reference(x, dy, w1, b1, w2, ALPHA)
    # the direct restatement and float64 autograd agree on both filter gradients (a check of the references, on the CPU)
    G2 = wgrad3d_ref(R["q32"].double(), dy.double(), ALPHA, -1, False)
    G1 = wgrad3d_ref(R["m32"].double(), x.double(), None, +1, True)
    assert (G2[:K, :27] - R["dW2"]).abs().max() <= 1e-9 * max(1.0, float(R["dW2"].abs().max()))
    assert (G1[:K, :27] - R["dW1"]).abs().max() <= 1e-9 * max(1.0, float(R["dW1"].abs().max()))
    assert (G1[:K, 27] - R["db1"]).abs().max() <= 1e-9 * max(1.0, float(R["db1"].abs().max()))
    nvox = B * D * H * W
    if integer:
        # everything lies on the grid of alpha = 0.25; every sum of |term|, in grid steps, stays below 2**24: exact in fp32
        qmax, mmax = float(R["q32"].abs().max()), float(R["m32"].abs().max())
        assert max(qmax, mmax) * 2 * nvox / ALPHA + 8 / ALPHA < EXACT_LIMIT                  # the 32 x 32 blocks (|x|, |dy| <= 2; + beta base)
        assert 27 * K * mmax / ALPHA < EXACT_LIMIT and float(R["dalpha_abs"]) < EXACT_LIMIT   # dx; dalpha
        assert int((R["q32"] == 0).sum()) > 0 or nvox * K < 8                                # the PReLU tie is in the data

    def cmp(got, ref, tol, what):
        if integer:
            exact(got, ref, f"{what} {c.name}")
        else:
            print(f"{what} {c.name}: max-rel {rel_err(got, ref)[0]:.3e} (bound {tol:g})")
            assert_close(got, ref, tol, f"{what} {c.name}")

    form = "four-voxel" if four(c) else "scalar"
    xg, xf = dev_buf(x, c.mis)
    dyg, dyf = dev_buf(dy, c.mis)
    w1g, b1g, w2g, ag = w1.cuda(), b1.cuda(), w2.cuda(), torch.tensor([ALPHA], device="cuda")
    hid = torch.empty(B, K, D, H, W)
    # ---- hidden_fwd: q = W1 * x + b1
    qg, qf = dev_buf(hid, c.mis, fill=NAN)
    assert L.cwfa_conv3d_hidden_fwd_f32(_p(xg), _p(w1g), _p(b1g), _p(qg), *dims, st) == 0
    torch.cuda.synchronize()
    assert untouched_outside(qg, qf) and untouched_outside(xg, xf)
    cmp(qg, R["q"], EW, f"q [{form}]")
    # ---- hidden_bwd from the reference's q rounded to fp32: m and dalpha (accumulated into 3.0); dalpha == NULL
    qin, _ = dev_buf(R["q32"], c.mis)
    mg, mf = dev_buf(hid, c.mis, fill=NAN)
    m2, _ = dev_buf(hid, c.mis, fill=NAN)
    dalpha = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
    assert L.cwfa_conv3d_hidden_bwd_f32(_p(dyg), _p(w2g), _p(qin), _p(ag), _p(mg), _p(dalpha), *dims, st) == 0
    assert L.cwfa_conv3d_hidden_bwd_f32(_p(dyg), _p(w2g), _p(qin), _p(ag), _p(m2), None, *dims, st) == 0
    torch.cuda.synchronize()
    assert untouched_outside(mg, mf) and untouched_outside(dyg, dyf)
    cmp(mg, R["m"], EW, f"m [{form}]")
    assert same_bits(mg, m2)
    if integer:
        exact(dalpha.cpu(), R["dalpha"] + 3.0, f"dalpha [{form}] {c.name}")
    else:
        # k: the 27 fp32 FMAs of W2^T * dy, the product with q, and the scalar kernel's fp32 running sum over its K channels
        # (the four-voxel kernel sums in double); the double block sum and atomics add < 2**-27
        assert_sum_bound(dalpha.cpu() - 3.0, R["dalpha"], R["dalpha_abs"], 27 + 1 + K + 1, f"dalpha [{form}] {c.name}")
    # ---- input_bwd from the reference's m rounded to fp32
    min_, _ = dev_buf(R["m32"], c.mis)
    dxg, dxf = dev_buf(x, c.mis, fill=NAN)
    assert L.cwfa_conv3d_input_bwd_f32(_p(min_), _p(w1g), _p(dxg), *dims, st) == 0
    torch.cuda.synchronize()
    assert untouched_outside(dxg, dxf)
    cmp(dxg, R["dx"], EW, f"dx [{form}]")
    # ---- wgrad: the two calls of ops.conv3d_1k1_backward (beta = 0 over NaN), and both with the other sign / bias / beta = 1
    blocks, items = c3_geom(c)
    nbytes = L.cwfa_conv3d_wgrad_workspace_bytes(B, D, H, W)
    assert nbytes == blocks * 16384, (c.name, "blocks restated", blocks, "workspace bytes", nbytes)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(_seed(c.name.removesuffix("_mis"), 7))
    pre = torch.randint(-8, 9, (32, 32), generator=g).float()
    # k: PReLU of the operand (1), the wave's fp32 accumulation in the matrix core (two products per step, 32 steps per item),
    # the reduction kernel's running sums over a quarter of the partials in four chains, and its two combining levels
    ipw = cdiv(items, 4 * blocks)
    k = 1 + 64 * ipw + cdiv(4 * blocks, 16) + 4
    for a_name, a_host, src_host, src_dev, alpha_dev in (("q", R["q32"], dy, dyg, ag), ("m", R["m32"], x, xg, None)):
        a_dev, _ = dev_buf(a_host, c.mis)
        for sign, want_bias, beta in ((-1, 0, 0.0), (+1, 1, 0.0), (+1, 1, 1.0), (-1, 0, 1.0)):
            what = f"wgrad(a = {a_name}, sign {sign:+d}, bias {want_bias}, beta {beta:g}) [{form}, {blocks} blocks, {items} items]"
            out = torch.full((32, 32), NAN, device="cuda") if beta == 0 else pre.cuda()
            assert L.cwfa_conv3d_wgrad_f32(_p(a_dev), _p(src_dev), _p(alpha_dev), _p(out), _p(ws), *dims, sign, want_bias, beta, st) == 0
            torch.cuda.synchronize()
            al = None if alpha_dev is None else ALPHA
            ref = wgrad3d_ref(a_host.double(), src_host.double(), al, sign, bool(want_bias)) + beta * pre.double()
            # rows >= K and columns >= 28 (27 without the bias column): zero, or what they held
            rest = torch.ones(32, 32, dtype=torch.bool)
            rest[:K, :27 + want_bias] = False
            assert torch.equal(out.cpu()[rest], (beta * pre)[rest]), what
            if integer:
                exact(out.cpu(), ref, f"{what} {c.name}")
            else:
                act = a_host.double() if al is None else torch.where(a_host > 0, a_host.double(), al * a_host.double())
                absterms = wgrad3d_ref(act.abs(), src_host.double().abs(), None, sign, bool(want_bias)) + beta * pre.double().abs()
                assert_sum_bound(out, ref, absterms, k, f"{what} {c.name}")
    return {"q": qg, "m": mg, "dx": dxg}


_c3_exact = {}


@pytest.mark.parametrize("c", C3_CASES, ids=_id)
def test_conv3d_backward_exact(c):
    """each of the four entry points, called as ops.conv3d_1k1_backward calls them, bit-equal to float64 on integer data; a W % 4 == 0
    shape from buffers one float past a 16-byte boundary (scalar kernels) bit-equal to the aligned run (four-voxel kernels)"""
    _c3_exact[c.name] = {k: v.cpu() for k, v in run_c3(c, True).items()}
    twin = c.name[:-4] if c.mis else None
    if twin in _c3_exact:
        for key, v in _c3_exact[c.name].items():
            assert same_bits(v, _c3_exact[twin][key]), (c.name, key)


@pytest.mark.parametrize("c", C3_CASES, ids=_id)
def test_conv3d_backward_rounding(c):
    """the same calls on random normal data: q, m, dx at 1e-6; dalpha and the 32 x 32 blocks per entry within k * 2**-24 * sum |term|"""
    run_c3(c, False)


# ------------------------------------------------------------------------------------------------ E. 3-D, empty and rejected calls
def test_conv3d_empty_batch():
    """B == 0: the per-voxel entry points write nothing; wgrad writes zeros (beta = 0) or leaves out32 bit-identical (beta = 1)"""
    from cwfa_amd import ops
    L, st = ops._lib.lib(), ops._stream()
    dims = (0, 2, 3, 4, 5)
    buf = [torch.full((256,), NAN, device="cuda") for _ in range(4)]
    w, al = torch.ones(5 * 27, device="cuda"), torch.tensor([ALPHA], device="cuda")
    dalpha = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
    assert L.cwfa_conv3d_hidden_fwd_f32(_p(buf[0]), _p(w), _p(w), _p(buf[1]), *dims, st) == 0
    assert L.cwfa_conv3d_hidden_bwd_f32(_p(buf[0]), _p(w), _p(buf[1]), _p(al), _p(buf[2]), _p(dalpha), *dims, st) == 0
    assert L.cwfa_conv3d_input_bwd_f32(_p(buf[2]), _p(w), _p(buf[3]), *dims, st) == 0
    torch.cuda.synchronize()
    assert all(b.isnan().all() for b in buf) and float(dalpha) == 3.0
    ws = torch.zeros(L.cwfa_conv3d_wgrad_workspace_bytes(*dims[:4]), dtype=torch.uint8, device="cuda")
    assert ws.numel() == 4096
    out = torch.full((32, 32), NAN, device="cuda")
    assert L.cwfa_conv3d_wgrad_f32(_p(buf[0]), _p(buf[1]), None, _p(out), _p(ws), *dims, 1, 1, 0.0, st) == 0
    assert same_bits(out, torch.zeros(32, 32, device="cuda"))
    pre = torch.randn(32, 32, device="cuda")
    out = pre.clone()
    assert L.cwfa_conv3d_wgrad_f32(_p(buf[0]), _p(buf[1]), _p(al), _p(out), _p(ws), *dims, -1, 0, 1.0, st) == 0
    assert same_bits(out, pre)


def test_conv3d_rejected_calls_touch_nothing():
    """K = 33, sign = 0, null pointers, bad shapes and the two 32-bit volume limits: the error code, and NaN-filled outputs as they
    were.  Every pointer is a real allocation at least as large as the arguments describe."""
    from cwfa_amd import ops
    L, st = ops._lib.lib(), ops._stream()
    B, D, H, W = 1, 2, 3, 4
    vol = B * D * H * W
    x, dy = torch.ones(vol, device="cuda"), torch.ones(vol, device="cuda")
    w, al = torch.ones(33 * 27, device="cuda"), torch.tensor([ALPHA], device="cuda")
    hid_in = torch.ones(33 * vol, device="cuda")
    outs = {k: torch.full((33 * vol,), NAN, device="cuda") for k in ("q", "m", "dx")}
    out32 = torch.full((32, 32), NAN, device="cuda")
    dalpha = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(L.cwfa_conv3d_wgrad_workspace_bytes(B, D, H, W), dtype=torch.uint8, device="cuda")

    def wg(a=hid_in, src=dy, out=out32, wsp=ws, dims=(B, D, H, W, 5), sign=1):
        return L.cwfa_conv3d_wgrad_f32(_p(a), _p(src), _p(al), _p(out), _p(wsp), *dims, sign, 1, 0.0, st)

    def fwd(xx=x, w1=w, b1=w, q=outs["q"], dims=(B, D, H, W, 5)):
        return L.cwfa_conv3d_hidden_fwd_f32(_p(xx), _p(w1), _p(b1), _p(q), *dims, st)

    def bwd(d=dy, w2=w, q=hid_in, a=al, m=outs["m"], dims=(B, D, H, W, 5)):
        return L.cwfa_conv3d_hidden_bwd_f32(_p(d), _p(w2), _p(q), _p(a), _p(m), _p(dalpha), *dims, st)

    def inp(m=hid_in, w1=w, dx=outs["dx"], dims=(B, D, H, W, 5)):
        return L.cwfa_conv3d_input_bwd_f32(_p(m), _p(w1), _p(dx), *dims, st)

    rejected = [
        ("wgrad K = 33", E_SHAPE, lambda: wg(dims=(B, D, H, W, 33))), ("wgrad sign = 0", E_INVAL, lambda: wg(sign=0)),
        ("wgrad sign = 2", E_INVAL, lambda: wg(sign=2)), ("wgrad a null", E_INVAL, lambda: wg(a=None)),
        ("wgrad src null", E_INVAL, lambda: wg(src=None)), ("wgrad out null", E_INVAL, lambda: wg(out=None)),
        ("wgrad workspace null", E_INVAL, lambda: wg(wsp=None)), ("wgrad K = 0", E_SHAPE, lambda: wg(dims=(B, D, H, W, 0))),
        ("wgrad W = 0", E_SHAPE, lambda: wg(dims=(B, D, H, 0, 5))), ("wgrad B < 0", E_SHAPE, lambda: wg(dims=(-1, D, H, W, 5))),
        ("fwd x null", E_INVAL, lambda: fwd(xx=None)), ("fwd w1 null", E_INVAL, lambda: fwd(w1=None)), ("fwd b1 null", E_INVAL, lambda: fwd(b1=None)),
        ("fwd q null", E_INVAL, lambda: fwd(q=None)), ("fwd D = 0", E_SHAPE, lambda: fwd(dims=(B, 0, H, W, 5))),
        ("bwd dy null", E_INVAL, lambda: bwd(d=None)), ("bwd w2 null", E_INVAL, lambda: bwd(w2=None)), ("bwd q null", E_INVAL, lambda: bwd(q=None)),
        ("bwd alpha null", E_INVAL, lambda: bwd(a=None)), ("bwd m null", E_INVAL, lambda: bwd(m=None)), ("bwd H = 0", E_SHAPE, lambda: bwd(dims=(B, D, 0, W, 5))),
        ("inp m null", E_INVAL, lambda: inp(m=None)), ("inp w1 null", E_INVAL, lambda: inp(w1=None)), ("inp dx null", E_INVAL, lambda: inp(dx=None)),
        ("inp K = 0", E_SHAPE, lambda: inp(dims=(B, D, H, W, 0))),
    ]
    for what, code, call in rejected:
        assert call() == code, what
    torch.cuda.synchronize()
    assert all(t.isnan().all() for t in outs.values()) and out32.isnan().all() and float(dalpha) == 3.0
    # B = 65536 > 65535 (the grid's y extent)
    Bb = 65536
    xb, hb = torch.ones(Bb, device="cuda"), torch.full((Bb,), NAN, device="cuda")
    ws1 = torch.zeros(L.cwfa_conv3d_wgrad_workspace_bytes(Bb, 1, 1, 1), dtype=torch.uint8, device="cuda")
    assert fwd(xx=xb, q=hb, dims=(Bb, 1, 1, 1, 1)) == E_SHAPE and inp(m=xb, dx=hb, dims=(Bb, 1, 1, 1, 1)) == E_SHAPE
    assert bwd(d=xb, q=xb, m=hb, dims=(Bb, 1, 1, 1, 1)) == E_SHAPE and wg(a=xb, src=xb, wsp=ws1, dims=(Bb, 1, 1, 1, 1)) == E_SHAPE
    torch.cuda.synchronize()
    assert hb.isnan().all() and out32.isnan().all()
    del xb, hb
    # the hidden volume K * D * H * W * 4 == 2**31 (K = 32 over 16 x 1024 x 1024: 2 GiB hidden, 64 MiB volumes)
    dims = (1, 16, 1024, 1024, 32)
    vol = 16 * 1024 * 1024
    small, small_out = torch.ones(vol, device="cuda"), torch.full((vol,), NAN, device="cuda")
    big = torch.full((32 * vol,), NAN, device="cuda")
    wsb = torch.zeros(L.cwfa_conv3d_wgrad_workspace_bytes(*dims[:4]), dtype=torch.uint8, device="cuda")
    assert fwd(xx=small, q=big, dims=dims) == E_SHAPE and bwd(d=small, q=big, m=big, dims=dims) == E_SHAPE
    assert inp(m=big, dx=small_out, dims=dims) == E_SHAPE and wg(a=big, src=small, wsp=wsb, dims=dims) == E_SHAPE
    # the volume D * H * W * 4 == 2**31 with K = 1 (the 2 GiB buffer serves as volume and as hidden volume)
    dims = (1, 512, 1024, 1024, 1)
    assert fwd(xx=big, q=big, dims=dims) == E_SHAPE and bwd(d=big, q=big, m=big, dims=dims) == E_SHAPE
    assert inp(m=big, dx=big, dims=dims) == E_SHAPE
    wsb = torch.zeros(L.cwfa_conv3d_wgrad_workspace_bytes(*dims[:4]), dtype=torch.uint8, device="cuda")
    assert wg(a=big, src=big, wsp=wsb, dims=dims) == E_SHAPE
    torch.cuda.synchronize()
    assert bool(big.isnan().all()) and bool(small_out.isnan().all()) and bool(out32.isnan().all()) and float(dalpha) == 3.0
