"""Evaluation helpers (reference: utils.py): ``psnr`` (:380-394), ``volume_2_projections`` (:281-327), ``norm_data`` /
``filter_data`` (:419-446).  The reductions over volumes are HIP kernels (csrc/eval_ops.hip); no torch operator runs on a volume.

``cwfa_amd.install()`` does NOT register this module as ``utils``: the reference's ``utils`` also holds its dataset loaders.
Inputs are assumed finite (the kernels do not propagate NaN)."""
import numpy as np
import torch

from . import _lib, ops
from .amp import amp_function

__all__ = ["psnr", "volume_2_projections", "norm_data", "filter_data"]


def _as_volume(t, name):
    """Any-shape device tensor as one [1, 1, 1, n] sample (contiguous tensors are viewed, not copied)."""
    ops._dev(t, name)
    return t.reshape(1, 1, 1, -1)


@amp_function
def psnr(img1, img2, PIXEL_MAX=1.0):
    """20 log10(PIXEL_MAX / sqrt(mean (img1 - img2)^2)); utils.py:380-394 with its two ``mse == 0`` branches (an int64 tensor [0] if
    img1 sums to zero, else [100]).  One pass over both tensors, sums in float64; returns a CPU float32 scalar tensor.
    Departure in a degenerate case only: ``img1.sum() == 0`` is decided by the float64 sum, the reference's by torch's fp32 sum --
    they differ only where a non-zero image cancels to exactly 0 in fp32."""
    a, b = _as_volume(img1, "img1"), _as_volume(img2, "img2")
    if a.numel() != b.numel():
        raise ValueError("psnr: the images differ in size")
    sse, s1 = ops.volume_metrics(b, a)[0, :2].tolist()                  # `gt` slot = img1: its sum decides the mse == 0 branch
    if sse == 0:
        return torch.tensor([0]) if s1 == 0 else torch.tensor([100])
    return torch.tensor(20.0 * np.log10(float(PIXEL_MAX) / np.sqrt(sse / a.numel())), dtype=torch.float32)


def depth_major(vol_in, depths_in_ch):
    """The [B, D, H, W] tensor behind the argument of ``volume_2_projections``: the argument itself with ``depths_in_ch``, else the
    depth-major tensor a [B, 1, H, W, D] argument is a ``permute(0,2,3,1).unsqueeze(1)`` view of (how the reference's loop passes
    every volume, CWFA.py:1081-1085).  A [B, 1, H, W, D] tensor stored depth-innermost would have to be transposed first."""
    ops._dev(vol_in, "vol_in")
    if depths_in_ch:
        if vol_in.dim() != 4:
            raise ValueError(f"volume_2_projections: depths_in_ch expects [B,D,H,W], got {tuple(vol_in.shape)}")
        return vol_in
    if vol_in.dim() != 5:
        raise ValueError(f"volume_2_projections: expected [B,1,H,W,D], got {tuple(vol_in.shape)}")
    if vol_in.shape[1] != 1:
        raise NotImplementedError("volume_2_projections: one channel only (every call of the reference passes one)")
    v = vol_in[:, 0].permute(0, 3, 1, 2)
    B, D, H, W = v.shape
    ok = (W == 1 or v.stride(3) == 1) and (H == 1 or v.stride(2) == W) and (D == 1 or v.stride(1) == H * W)
    if not ok:
        raise NotImplementedError("volume_2_projections: a [B,1,H,W,D] argument must be a permuted view of a depth-major [B,D,H,W] "
                                  "tensor (vol.permute(0,2,3,1).unsqueeze(1)); pass the [B,D,H,W] tensor with depths_in_ch=True instead")
    return v


def compose_projections(zp, xp, yp, scaling_factors, border_thickness, add_scale_bars):
    """Composite images [B, 1, H', W'] from the three projections of ``ops.mip3``; the fill value is the minimum of the over-depth
    image over the whole batch (``z_projection.min()``, utils.py:312), found by the extrema kernel."""
    B, H, W = zp.shape
    fill = ops.volume_extrema(zp.reshape(1, 1, 1, -1))[0, 0:1]
    out = ops.projection_compose(zp, xp, yp, fill, scaling_factors[2], border_thickness, add_scale_bars)
    return out.unsqueeze(1)


def check_layout(shape, scaling_factors):
    if len(scaling_factors) != 3 or int(scaling_factors[0]) != 1 or int(scaling_factors[1]) != 1 or int(scaling_factors[2]) < 1:
        raise ValueError(f"volume_2_projections: scaling_factors {list(scaling_factors)}: the plane cannot be scaled (the reference "
                         "stores the unscaled over-depth image into the scaled slot and fails), the depth factor must be >= 1")
    if shape[2] != shape[3]:
        raise ValueError(f"volume_2_projections: H = {shape[2]} != W = {shape[3]}: the reference sizes the over-H image by H, stores "
                         "it W wide and fails; only square planes have a composite")


@amp_function
def volume_2_projections(vol_in, proj_type=torch.amax, scaling_factors=[1, 1, 2], depths_in_ch=False, ths=[0.0, 1.0],
                         normalize=False, border_thickness=2, add_scale_bars=False, scale_bar_vox_sizes=[40, 20], on_device=False):
    """The composite of the three maximum projections of |vol_in|; utils.py:281-327, same signature.  Returns a CPU float32
    tensor [B, 1, H + D*s + border, W + D*s + border] like the reference; ``on_device=True`` keeps it on the GPU.

    One read of the volume (``ops.mip3``); ``normalize`` and non-default ``ths`` cost one extrema pass before it, and their maps
    (normalise, lower threshold, upper clamp) are applied to every voxel on load, in the reference's fp32 operations and order,
    so the result is bit-exact.  ``proj_type`` other than ``torch.amax`` raises NotImplementedError."""
    if proj_type is not torch.amax:
        raise NotImplementedError("volume_2_projections: proj_type must be torch.amax (the maximum projection)")
    v = depth_major(vol_in, depths_in_ch)
    check_layout(v.shape, scaling_factors)
    post = None
    thresholds = ths[0] != 0.0 or ths[1] != 1.0
    if normalize or thresholds:
        ext = ops.volume_extrema(v).cpu()
        lo, hi = ext[:, 2].min(), ext[:, 3].max()                      # fp32 scalars: vol.min(), vol.max() of |vol_in|
        post = _lib.EvalPost()
        if normalize:                                                  # vol -= vol.min(); vol /= vol.max()
            div = hi - lo
            post.normalize, post.norm_sub, post.norm_div = 1, float(lo), float(div)
            lo, hi = (lo - lo) / div, (hi - lo) / div                  # the maps are monotone: the extrema map with them
        if thresholds:
            rng = hi - lo
            post.threshold, post.vol_min = 1, float(lo)
            post.lower, post.upper, post.clamp_value = float(rng * ths[0]), float(rng * ths[1]), float(lo + rng * ths[1])
    zp, xp, yp, _ = ops.mip3(v, post=post)
    out = compose_projections(zp, xp, yp, scaling_factors, border_thickness, add_scale_bars)
    return out if on_device else out.cpu()


def filter_data(data, kernel_size=10):
    """Moving average, ``np.convolve(data, ones(k) / k, mode='same')``; utils.py:419-427.  Host numpy on a [T] vector."""
    kernel = np.ones(kernel_size) / kernel_size
    return np.convolve(np.asarray(data, dtype=np.float64), kernel, mode="same")


def norm_data(data, filter=10):
    """(d - min d) / max d of the (filtered) trace and its range max - min; utils.py:429-446 -- the division is by the maximum
    BEFORE the minimum is subtracted, as there.  Host numpy (float64) on a [T] vector."""
    d1 = np.asarray(data, dtype=np.float64) * 1.0
    if filter != 0:
        d1 = filter_data(d1, filter)
    min_d1, max_d1 = np.min(d1), np.max(d1)
    m_d1 = max_d1 if max_d1 != 0 else 1
    return (d1 - min_d1) / m_d1, max_d1 - min_d1
