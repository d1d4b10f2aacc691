"""Helpers of the fused split layer's dispatch tests (a plain module, not a conftest): an integer data set on which every form of
csrc/conv_split_layer.hip must give the fp32 bits of float64, the host selection of layer_launch restated, the channel-blocked
layout, and the geometry of the persistent-walk cases.

Exact data.  y = ELU(W1 . ELU(conv3x3(x, W3) + b3) + b1 + x) with x = conv1x1(u, W0) + b0, 64 channels:
  u    integers in {-1, 0, 1}, [B, cin, H, W]
  w0   2 non-zeros of +-1 per output row, b0 in {-1, 0, 1}: x is an integer with |x| <= 3 (the input of the plain forms, the residual
       of the first-layer forms)
  w3   24 non-zeros from {+-1, +-2} per output channel: |conv3x3(x)| <= S3 = 2 * 24 * 3 = 144
  b3   +S3; channels c % 8 == 5: -(S3 + 20), the saturated branch
  w1   8 non-zeros of +-1 per row
  b1   +S1 with S1 = 8 * HID_MAX + 3; channels c % 8 == 2: -(S1 + 20).  HID_MAX = 256 is the asserted bound on the hidden map (the
       largest run of integers bf16 holds exactly), not the maximum measured on one data set: b1 then does not depend on the data,
       which the walk cases need -- their float64 reference covers one sample of four.
Every operand, and every entry of the composed bank of ops.pack_first_layer_weight, is an integer of at most 8 significant bits:
exact as one bf16, one fp16 or three bf16 pieces.  Every partial sum is an integer far below 2^24: exact in fp32 in any order.  Both
ELUs are exact: the pre-activation is >= 0, where med3(v, exp(v) - 1, 0) = v (also when exp overflows to inf), or <= -20, where
exp(v) - 1 rounds to -1.0f in fp32 as it does when float64 is rounded to fp32.  `check_premises` asserts all of this on the float64
reference, so a later change to the recipe cannot quietly make the tests inexact."""
import torch
import torch.nn.functional as F

S3 = 2 * 24 * 3
HID_MAX = 256
S1 = 8 * HID_MAX + 3
SAT = 20                                    # |pre-activation| of the saturated branch is at least this


# ------------------------------------------------------------------------------------------------ channel-blocked maps
def _to_blocked(t):
    """[B,64,H,W] NCHW -> the same tensor object shape holding [B][C/8][H][W][8]"""
    B, Cc, H, W = t.shape
    return t.view(B, Cc // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().view(B, Cc, H, W)


def _from_blocked(t):
    B, Cc, H, W = t.shape
    return t.reshape(B, Cc // 8, H, W, 8).permute(0, 1, 4, 2, 3).contiguous().view(B, Cc, H, W)


# ------------------------------------------------------------------------------------------------ the host selection, restated
# split_layer_kernel<SIX, INB, OUTB, NPER, TAPE, XF, SHORT, F16>: the 13 (NPER, TAPE, XF, SHORT, INB, OUTB) that layer_launch /
# layer_form build in each operand format (SIX, F16) = (1, 0) split_bf16 | (0, 0) bf16 | (0, 1) fp16
FORMATS = ("split_bf16", "bf16", "fp16")
ALL_FORMS = frozenset(
    [(2, False, False, False, bool(l & 1), bool(l & 2)) for l in range(4)]          # cwfa_subnet_layer_split_f32
    + [(2, True, False, False, False, False)]                                         # cwfa_subnet_layer_split_tape_f32
    + [(1, False, False, False, bool(l & 1), bool(l & 2)) for l in range(4)]        # cwfa_subnet_layer_first_f32, x given
    + [(1, False, True, False, False, bool(l & 2)) for l in (0, 2)]                 # ... x = NULL, long image
    + [(1, False, True, True, False, bool(l & 2)) for l in (0, 2)])                 # ... x = NULL, layout | 4
assert len(ALL_FORMS) == 13


def select(entry, layout=0, x_none=False, short=False, hid=False, u_ch=0):
    """(entry point "plain" | "tape" | "first", layout & 3, x is NULL, the short bit, a hidden map is asked for) ->
    (NPER, TAPE, XF, SHORT, INB, OUTB) as layer_launch selects it, or None where the host code rejects the call"""
    if layout < 0 or layout > 3:
        return None
    if entry == "tape":                                       # tape: NCHW only (the entry point has no layout argument)
        return (2, True, False, False, False, False) if hid and layout == 0 and not short and not x_none else None
    if hid:
        return None
    if entry == "plain":                                      # no u: no short bit, x is required
        return None if short or x_none else (2, False, False, False, bool(layout & 1), bool(layout & 2))
    assert entry == "first"
    if not 1 <= u_ch <= 32 or (short and (not x_none or u_ch > 16)):
        return None
    if x_none:
        layout &= 2                                           # (no x: its layout bit means nothing)
    return (1, False, x_none, short, bool(layout & 1), bool(layout & 2))


# ------------------------------------------------------------------------------------------------ exact data
def compose_first_layer(w0, b0, w3):
    """the bank of ops.pack_first_layer_weight restated: w3c[o][i][tap] = sum_m w3[o][m][tap] [w0 | b0][m][i] and w0c = [W0 | b0 | 0]
    (float64, rounded once), both zero-padded to 32 input channels"""
    cin = w0.shape[1]
    w0p = torch.cat([w0.reshape(64, cin).double(), b0.double().reshape(64, 1)], 1)
    w3c = torch.zeros(64, 32, 3, 3)
    w3c[:, :cin + 1] = torch.einsum("omt,mi->oit", w3.double().reshape(64, 64, 9), w0p).reshape(64, cin + 1, 3, 3).float()
    w0c = torch.zeros(64, 32)
    w0c[:, :cin + 1] = w0p.float()
    return w3c, w0c


def _sparse_rows(g, rows, cols, nnz, values):
    """[rows, cols] with nnz non-zeros per row drawn from `values`"""
    pos = torch.rand(rows, cols, generator=g).argsort(1)[:, :nnz]
    val = torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), (rows, nnz), generator=g)]
    return torch.zeros(rows, cols).scatter_(1, pos, val), pos, val


def exact_weights(cin, seed):
    """the banks and biases of the recipe (CPU, fp32); `w0_pos` / `w0_val`: the two non-zeros of each row of w0"""
    assert 2 <= cin <= 31
    g = torch.Generator().manual_seed(seed)
    w0, pos, val = _sparse_rows(g, 64, cin, 2, (-1.0, 1.0))
    b0 = torch.randint(-1, 2, (64,), generator=g).float()
    w3 = _sparse_rows(g, 64, 64 * 9, 24, (-2.0, -1.0, 1.0, 2.0))[0].view(64, 64, 3, 3)
    w1 = _sparse_rows(g, 64, 64, 8, (-1.0, 1.0))[0].view(64, 64, 1, 1)
    c = torch.arange(64)
    b3 = torch.where(c % 8 == 5, -float(S3 + SAT), float(S3))
    b1 = torch.where(c % 8 == 2, -float(S1 + SAT), float(S1))
    return {"w0": w0.view(64, cin, 1, 1), "b0": b0, "w3": w3, "b3": b3, "w1": w1, "b1": b1, "w0_pos": pos, "w0_val": val, "cin": cin}


def first_map(u, wt):
    """x = conv1x1(u, w0) + b0 as two gathers and two additions on u's device: small integers, exact in fp32 in any order"""
    pos, val = wt["w0_pos"].to(u.device), wt["w0_val"].to(u.device)
    x = u[:, pos[:, 0]] * val[:, 0].view(1, 64, 1, 1)
    x += u[:, pos[:, 1]] * val[:, 1].view(1, 64, 1, 1)
    x += wt["b0"].to(u.device).view(1, 64, 1, 1)
    return x


def reference(x, wt):
    """float64 (hidden, y) of the layer on the CPU, with both pre-activations"""
    x = x.detach().cpu().double()
    pre3 = F.conv2d(x, wt["w3"].double(), wt["b3"].double(), padding=1)
    hidden = F.elu(pre3)
    pre1 = F.conv2d(hidden, wt["w1"].double(), wt["b1"].double()) + x
    return {"pre3": pre3, "hidden": hidden, "pre1": pre1, "y": F.elu(pre1)}


def _bf16_exact(t):
    return torch.equal(t.bfloat16().float(), t.float())


def check_premises(d):
    """the premises of bit-exactness, asserted on the data and its float64 reference (see the module docstring)"""
    wt, r = d["wt"], d["ref"]
    for name in ("pre3", "pre1"):
        v = r[name]
        assert bool(((v >= 0) | (v <= -SAT)).all()), (name, "a pre-activation between -20 and 0")
    assert float(r["hidden"].max()) <= HID_MAX, ("hidden map", float(r["hidden"].max()))
    w3c, w0c = compose_first_layer(wt["w0"], wt["b0"], wt["w3"])
    for name, t in (("u", d["u"]), ("x", d["x"]), ("w0", wt["w0"]), ("w3", wt["w3"]), ("w1", wt["w1"]), ("w3c", w3c), ("w0c", w0c)):
        assert _bf16_exact(t.detach().cpu()), (name, "changed by a bf16 round trip")
    assert float(d["x"].abs().max()) <= 3 and float(w3c.abs().max()) <= HID_MAX
    for name in ("hidden", "y"):
        v = r[name].float()
        assert torch.equal(v, v.round()), (name, "float64 rounded to fp32 is not the integer result")
        assert float((v == -1).float().mean()) >= 0.10, (name, "less than 10 % on the -1 branch")
        assert not bool((v == -1).all())
    # y takes many values (an error cannot hide in a constant map): more than 1000 where the map has room for them; the smallest
    # shapes of the case list have 128 .. 960 elements, an eighth of them on the -1 branch: a quarter of the count there
    n, distinct = r["y"].numel(), r["y"].float().unique().numel()
    assert distinct > (1000 if n >= 8192 else n // 4), ("distinct values of y", distinct, n)
    return d


def exact_layer_data(B, cin, H, W, seed=0, device="cpu", ref_samples=None):
    """-> {"u" [B,cin,H,W], "x" [B,64,H,W] (fp32, on `device`), "wt" (exact_weights), "ref" (float64 reference of samples `ref_samples`,
    default all, CPU), "ref_samples"}; the premises are asserted before it returns"""
    wt = exact_weights(cin, 1000 * seed + cin)
    g = torch.Generator(device=device).manual_seed(seed * 7919 + B * 31 + H * 1009 + W)
    u = torch.randint(-1, 2, (B, cin, H, W), generator=g, device=device).float()
    x = first_map(u, wt)
    sl = slice(None) if ref_samples is None else ref_samples
    d = {"u": u, "x": x, "wt": wt, "ref_samples": sl}
    d["ref"] = reference(x[sl], wt)
    check_premises({**d, "u": u[sl], "x": x[sl]})
    return d


# ------------------------------------------------------------------------------------------------ persistent walk
def walk_geometry(n_cu, second=False):
    """(B, H, W, tiles per sample T, tiles in all) of the walk cases on a device with n_cu compute units (one persistent workgroup
    each).  First geometry: 8 tile rows (H = 123), tiles_x = n_cu // 10, so T = 8 tiles_x is a multiple of 8 (the XCD tile map is on)
    and T <= n_cu (a sample launched alone has one tile per workgroup: no walk); W leaves the last tile column ragged; B is the
    smallest batch with B T >= 3 n_cu + 8: every workgroup walks at least three tiles.  Second geometry: 7 tile rows and four more
    tile columns -- a tile count that is no multiple of 8, so the walk runs unmapped under the default option."""
    tiles_y, tiles_x = (7, n_cu // 10 + 4) if second else (8, n_cu // 10)
    T = tiles_y * tiles_x
    B = -(-(3 * n_cu + 8) // T)
    return B, 16 * tiles_y - 5, 32 * tiles_x - 9, T, B * T


def walk_premises(n_cu, second=False):
    """what the walk cases rely on; asserted (a failure, not a skip) by the tests"""
    B, H, W, T, total = walk_geometry(n_cu, second)
    assert n_cu % 8 == 0, n_cu                                  # gridDim.x = n_cu: the tile map needs it a multiple of 8
    assert 0 < T <= n_cu, (T, n_cu)                             # alone: no walk
    assert total >= 3 * n_cu + 8, (total, n_cu)                 # batched: every workgroup walks >= 3 tiles, >= 8 walk one more
    assert (-(-H // 16), -(-W // 32)) == ((7, T // 7) if second else (8, T // 8))
    assert (total % 8 != 0) if second else (total % 8 == 0 and T % 8 == 0), (total, T)
    assert 64 * H * W * 4 < 2 ** 31
    return B, H, W, T, total
