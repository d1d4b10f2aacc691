"""Autocast entry of the modules.  The reference runs its reconstruction, evaluation and training loops under
``torch.cuda.amp.autocast`` by default (``--use_half_precision 1``).  Here the arithmetic of the convolutions is chosen once,
process-wide, by ``ops.set_precision`` (``"fp16"`` is what autocast does on a GPU); an autocast region must not change it.  So
every module ``forward`` goes through ``amp_entry``: inside an autocast region it upcasts fp16 / bf16 tensor arguments to fp32
and runs with autocast disabled, so that the host-side torch products of the modules (the Householder mix of AllInOneBlock,
for one) stay fp32 and the outputs are what the same call returns outside the region.  Outside a region it calls straight
through.  (ops.* itself stays strict: it rejects non-fp32 tensors.)"""
import functools

import torch

__all__ = ["amp_entry", "amp_function", "amp_region"]


def _up(v):
    if torch.is_tensor(v):
        return v.float() if v.dtype in (torch.float16, torch.bfloat16) else v
    if isinstance(v, (list, tuple)):
        return type(v)(_up(t) for t in v)
    return v


def amp_entry(forward):
    """Decorator for a module's ``forward`` (see the module docstring)."""
    @functools.wraps(forward)
    def wrapped(self, *args, **kwargs):
        if not torch.is_autocast_enabled("cuda"):
            return forward(self, *args, **kwargs)
        with torch.autocast("cuda", enabled=False):
            return forward(self, *_up(args), **{k: _up(v) for k, v in kwargs.items()})
    return wrapped


def amp_function(fn):
    """``amp_entry`` for a plain function (the evaluation mirrors of ``utils`` and ``CWFA``)."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        if not torch.is_autocast_enabled("cuda"):
            return fn(*args, **kwargs)
        with torch.autocast("cuda", enabled=False):
            return fn(*_up(args), **{k: _up(v) for k, v in kwargs.items()})
    return wrapped


def amp_region(fn):
    """``amp_function`` without the upcast, for the data preparation mirrors: their fp16 volumes are data in the reference's own
    storage format (XLFMDatasetFull keeps them in fp16), not autocast products, and the kernels read them as fp16."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        if not torch.is_autocast_enabled("cuda"):
            return fn(*args, **kwargs)
        with torch.autocast("cuda", enabled=False):
            return fn(*args, **kwargs)
    return wrapped
