"""The reference's optimiser on the HIP kernels: ``Lion`` (``from lion_pytorch import Lion``, CWFA.py:24,381,608-610) as a
``torch.optim.Optimizer`` whose ``step()`` is one launch of ``cwfa_lion_step_f32`` per 96 parameter tensors.

Update rule (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms", with decoupled weight decay, in the order
``lion_pytorch`` applies it), per element with g the gradient and m the state ``exp_avg``:

    p <- p * (1 - lr * wd);  p <- p - lr * sign(beta1 * m + (1 - beta1) * g);  m <- beta2 * m + (1 - beta2) * g

AMP: the class declares ``_step_supports_amp_scaling``.  ``torch.amp.GradScaler.step`` then does not unscale the gradients and
does not decide on the host whether to skip the step: it sets ``optimizer.grad_scale`` / ``optimizer.found_inf`` (device tensors)
around the call, and ``step()`` hands both to the kernel, which divides every gradient by the scale as it reads it and writes
nothing when ``found_inf`` is set.  After an explicit ``scaler.unscale_(optimizer)`` the scale arrives as ``None`` (the gradients
are unscaled already).  Nothing in ``step()`` waits for the device."""
import torch

from . import ops

__all__ = ["Lion"]


class Lion(torch.optim.Optimizer):
    """``Lion(params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0)``; ``params``: parameters, or group dicts with their own
    ``lr`` / ``betas`` / ``weight_decay`` (CWFA.py:603-610).  State per parameter: ``exp_avg`` (the key ``lion_pytorch`` uses, so
    the ``optimizer_state_dict`` of its checkpoints loads), created as zeros by the first step that sees a gradient.  fp32 parameters
    on a HIP device only (no CPU fallback exists)."""

    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0):
        if not lr > 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
            raise ValueError(f"Invalid beta parameters: {betas}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), weight_decay=weight_decay))
        for group in self.param_groups:                     # per-group values get the same checks as the defaults
            if not group["lr"] > 0.0:
                raise ValueError(f"Invalid learning rate: {group['lr']}")
            if len(group["betas"]) != 2 or not all(0.0 <= float(b) < 1.0 for b in group["betas"]):
                raise ValueError(f"Invalid beta parameters: {group['betas']}")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)    # set by GradScaler.step
        for group in self.param_groups:
            ps, gs, ms = [], [], []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("Lion does not support sparse gradients")
                if not (p.is_contiguous() and g.is_contiguous()):
                    raise RuntimeError(f"Lion: a parameter of shape {tuple(p.shape)} or its gradient is not contiguous; the fused "
                                       "update works in place on contiguous tensors")
                state = self.state[p]
                m = state.get("exp_avg")
                if m is None:
                    m = state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                ps.append(p)
                gs.append(g)
                ms.append(m)
            ops.lion_step(ps, gs, ms, group["lr"], group["betas"], group["weight_decay"], grad_scale, found_inf)
        return loss
