"""Case list and input builder shared by tests/test_gpu_split3x3_midstep.py and tools/make_split3x3_bits.py (a plain module, not a
conftest): the launches of csrc/conv_split3x3.hip at which the step schedule -- two weight slots, one barrier per step, the
pre-read of the next step's fragments -- can go wrong, each as one `Case` that runs a handful of launch variants.

  * input channels 16 (one chunk: five steps, the loop ends right after a pre-read), 48 (odd chunk count: the trailing all-zero steps
    are skipped), 64 (two periods: a step's slot is its parity and a period has nine steps, so both slot parities), 96 (three
    periods: the staging set serves even, odd, even, ... chunks);
  * images of one tile and of partial tiles both ways: 8 x 32 and 24 x 40, for the 16-row forms 16 x 32 and 40 x 40;
  * batch 2 (blockIdx.z).
Inputs are built as tests/test_gpu_split3x3_onepass.py builds them, for the reasons given there: x, the affine tables and the skip
tensor on a dyadic grid, weights scaled by 2^(-3 .. 3) per (filter, channel)."""
import hashlib
import zlib
from dataclasses import dataclass

import torch

from split_ref import pack_split3x3, pack_split7x7

B = 2
CINS = (16, 48, 64, 96)
IMAGES8 = ((8, 32), (24, 40))
IMAGES16 = ((16, 32), (40, 40))
PROS = tuple((aff, add) for aff in (False, True) for add in (False, True))
GOLDEN_NAME = "g28_split3x3_parent_bits.json"


@dataclass(frozen=True)
class Case:
    form: str                 # see FORMS
    cin: int
    H: int
    W: int

    @property
    def name(self):
        return f"{self.form}_cin{self.cin}_{self.H}x{self.W}"


# form -> (bank size, images, input channels, operand formats)
FORMS = {
    "c256": (512, IMAGES8, CINS, ("split_bf16", "bf16", "fp16")),   # MPW 4: 256 and 512 outputs x (affine, skip add), PReLU, out_stats
    "c96": (96, IMAGES16, CINS, ("split_bf16", "bf16")),            # MPW 3, WM 2
    "c64": (64, IMAGES16, CINS, ("split_bf16", "bf16")),            # no prologue: 16-row form, two m-tiles x two channel groups
    "c64a": (64, IMAGES8, CINS, ("split_bf16", "bf16")),            # load-side affine: the 8-row form
    "c48": (48, IMAGES16, CINS, ("split_bf16", "bf16")),            # narrow tilings, WM 1
    "c12": (12, IMAGES16, CINS, ("split_bf16", "bf16")),
    "couple": (24, IMAGES8, (64,), ("split_bf16", "bf16")),         # coupling epilogue, 64 -> 24 pairs (8-row and 16-row form)
    "k7": (64, IMAGES8, (64,), ("split_bf16", "bf16")),             # 7x7 over 64 channels
}
CASES = [Case(f, cin, H, W) for f, (_, images, cins, _) in FORMS.items() for cin in cins for H, W in images]
PARAMS = [(c, fmt) for c in CASES for fmt in FORMS[c.form][3]]
PARAM_IDS = [f"{c.name}-{fmt}" for c, fmt in PARAMS]

_INPUTS = {}


def inputs(c):
    """seeded CPU tensors of a case (shared by every operand format and never modified)"""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    bank = FORMS[c.form][0]

    def dy(*s):
        return torch.randint(-127, 128, s, generator=g).float() / 16

    if c.form == "couple":          # (as tests/test_gpu_split_dispatch.py: s stays where the soft clamp is not saturated)
        t = {"x": torch.randn(B, c.cin, c.H, c.W, generator=g), "w": torch.randn(2 * bank, c.cin, 3, 3, generator=g) * (1.5 / (3 * c.cin ** 0.5)),
             "b": torch.randn(2 * bank, generator=g) * 0.1, "xh": torch.randn(B, bank, c.H, c.W, generator=g)}
    else:
        ks = 7 if c.form == "k7" else 3
        w = torch.randn(bank, c.cin, ks, ks, generator=g) / (ks * ks * c.cin) ** 0.5
        w = w * 2.0 ** torch.randint(-3, 4, (bank, c.cin, 1, 1), generator=g).float()
        t = {"x": dy(B, c.cin, c.H, c.W), "w": w, "b": torch.randn(bank, generator=g),
             "alpha": torch.randint(-4, 9, (bank,), generator=g).float() / 8,
             "sc": 2.0 ** torch.randint(-1, 2, (B, c.cin), generator=g).float(), "sh": dy(B, c.cin), "add": dy(B, c.cin, c.H, c.W)}
    _INPUTS[c.name] = t
    return t


def run_case(ops, c, fmt):
    """Every launch variant of case c in operand format fmt (ops.set_precision(fmt) is the caller's).
    -> {variant: dict(y=..., and per variant: cout, aff, add, act, stats, logdet)}; the variants whose output is also compared by
    digest are those without a "nodigest" entry."""
    t = inputs(c)
    dev = {k: v.cuda() for k, v in t.items()}
    out = {}
    if c.form == "couple":
        bank = ops.pack_couple_weight(dev["w"], dev["b"])
        assert bank[0].split
        y = torch.empty(B, FORMS[c.form][0], c.H, c.W, device="cuda")
        ld = torch.zeros(B, dtype=torch.float64, device="cuda")
        ops.conv3x3_couple(dev["x"], bank, dev["xh"], y, "ATAN", 1.7, 1.0, False, logdet=ld)
        out["fwd"] = dict(y=y, logdet=ld)
        return out
    if c.form == "k7":
        pc = pack_split7x7(ops, dev["w"])
        assert pc.split and pc.ks == 7
        out["bias"] = dict(y=ops.conv2d(dev["x"], pc, bias=dev["b"]), cout=64, aff=False, add=False, act=None)
        return out
    if c.form == "c256":
        couts = (256,) if fmt == "fp16" else (256, 512)
        for cout in couts:
            pc = pack_split3x3(ops, dev["w"][:cout].contiguous())
            assert pc.split
            bias, alpha = dev["b"][:cout].contiguous(), dev["alpha"][:cout].contiguous()
            for aff, add in PROS:
                kw = dict(bias=bias, act="prelu", prelu_alpha=alpha, in_scale=dev["sc"] if aff else None, in_shift=dev["sh"] if aff else None,
                          in_add=dev["add"] if add else None)
                tag = f"cout{cout}_aff{int(aff)}_add{int(add)}"
                out[tag] = dict(y=ops.conv2d(dev["x"], pc, **kw), cout=cout, aff=aff, add=add, act="prelu")
                if cout == 512:         # two cout tiles: the plain block order computes the same bits
                    ops.set_option("split3x3_xcd_map", 0)
                    try:
                        out[tag + "_plainorder"] = dict(y=ops.conv2d(dev["x"], pc, **kw), same_as=tag, nodigest=True)
                    finally:
                        ops.set_option("split3x3_xcd_map", 1)
                else:                   # with the BatchNorm statistics of the output (float64 atomics: not bit-stable, y is)
                    st = torch.zeros(2 * cout, dtype=torch.float64, device="cuda")
                    out[tag + "_stats"] = dict(y=ops.conv2d(dev["x"], pc, out_stats=st, **kw), same_as=tag, stats=st, nodigest=True)
        return out
    cout = FORMS[c.form][0]
    pc = pack_split3x3(ops, dev["w"])
    assert pc.split
    aff = c.form == "c64a"
    for act in (None, "prelu"):
        out["prelu" if act else "bias"] = dict(
            y=ops.conv2d(dev["x"], pc, bias=dev["b"], act=act, prelu_alpha=dev["alpha"] if act else None,
                         in_scale=dev["sc"] if aff else None, in_shift=dev["sh"] if aff else None),
            cout=cout, aff=aff, add=False, act=act)
    return out


def digest(y):
    """SHA-256 of the output's bytes (contiguous, in memory order)"""
    return hashlib.sha256(y.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def key(c, fmt, variant):
    return f"{fmt}/{c.name}/{variant}"
