"""The reference's ``losses`` module as far as CWFA.py uses it: ``weighted_mse_loss`` (the `wL2` choice of --loss_func_first_step /
--loss_func_reg, CWFA.py:941-942,955), on the fused HIP pass of DESIGN.md section 15.  ``cwfa_amd.install(losses=True)`` registers
this module under the name ``losses``, so that the reference's ``import losses as Losses`` resolves to it.  It holds only what CWFA.py
uses from losses.py: none of that file's other (time-series) losses exist here.
"""
import torch
from torch.autograd.function import once_differentiable

from . import ops

__all__ = ["weighted_mse_loss"]


class _WeightedMSE(torch.autograd.Function):
    """forward: the extrema pass and the loss pass; the one gradient map d loss / d output is kept (the target's is its negative).
    The masks are comparisons: they carry no gradient, as the reference's ``.float()`` of a comparison carries none."""

    @staticmethod
    def forward(ctx, output, target, ths_perc, need):
        numel = output.numel()
        out, gmap = ops.wmse_loss(output.detach().contiguous(), target.detach().contiguous(), ths_perc,
                                  gscale=1.0 / max(numel, 1), want_grad=need)
        ctx.gmap = gmap
        return (out[0] / numel).to(torch.float32)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gmap, ctx.gmap = ctx.gmap, None
        a = float(g)
        go = ops.axpby(gmap, a) if ctx.needs_input_grad[0] else None
        gt = ops.axpby(gmap, -a) if ctx.needs_input_grad[1] else None
        return go, gt, None, None


def weighted_mse_loss(output, target, ths_perc=0.05):
    """mean((output - target)^2 * m_o * m_t) with m_v = (v - min v) > (max v - min v) * ths_perc: the MSE over the elements brighter than
    ``ths_perc`` of the range in both tensors, divided by the number of ALL elements.  fp32 tensors of one shape on the HIP device;
    returns a 0-dim fp32 tensor.  Differentiable in both arguments (once); under ``torch.no_grad()`` no gradient map is written."""
    # (inside forward() the grad mode is always off and needs_input_grad ignores no_grad: whether a graph is recorded is decided here)
    need = torch.is_grad_enabled() and bool(getattr(output, "requires_grad", False) or getattr(target, "requires_grad", False))
    return _WeightedMSE.apply(output, target, float(ths_perc), need)
