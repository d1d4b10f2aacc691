"""Evaluation helpers (reference: utils.py): ``psnr`` (:380-394), ``volume_2_projections`` (:281-327), ``norm_data`` /
``filter_data`` (:419-446), and the data preparation in front of a run: ``fast_quantile`` (:84-102), ``crop_volume_center``
(:105-126), ``load_process_volume`` (:128-184) and ``prepare_XLFM_data``, the body of ``load_XLFM_data`` (:187-220) behind the
dataset object.  The passes over volumes are HIP kernels (csrc/eval_ops.hip, csrc/prep_ops.hip); no torch operator runs on a volume.

``cwfa_amd.install()`` does NOT register this module as ``utils``: the reference's ``utils`` also holds its dataset loaders.
Inputs are assumed finite (the kernels do not propagate NaN)."""
import numpy as np
import torch

from . import _lib, ops
from .amp import amp_function, amp_region

__all__ = ["psnr", "volume_2_projections", "norm_data", "filter_data", "fast_quantile", "crop_volume_center", "load_process_volume",
           "prepare_XLFM_data"]


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


# ------------------------------------------------------------------------------------------------ data preparation
QUANTILE_BINS = 10000


def quantile_walk(counts, edges, quant):
    """The host half of ``fast_quantile``: the reference's walk over the bins above bin 0, in its fp32 arithmetic.  ``counts``: the
    histogram as a float32 CPU tensor (what torch.histogram returns), ``edges`` float32 [bins+1].  The walk stops at the first bin
    whose preceding bins (1 .. n-1) already hold ``sum(counts[1:]) * quant`` elements and returns that bin's lower edge; when
    nothing crosses it ends on the last bin, ``edges[bins-1]`` -- not the maximum."""
    h = counts.to(torch.float32)
    bins = h.numel()
    if bins < 2:
        raise ValueError("fast_quantile: needs at least two bins (the reference's walk starts at bin 1)")
    target = np.float32(h[1:].sum() * quant)                              # torch's fp32 sum and product, as there
    before = np.zeros(bins - 1, dtype=np.float32)                         # before[i]: the sequential fp32 sum of bins 1 .. i
    np.cumsum(h[1:bins - 1].numpy(), dtype=np.float32, out=before[1:])
    hit = np.nonzero(before >= target)[0]
    n_bin = int(hit[0]) + 1 if len(hit) else bins - 1
    return edges[n_bin]


@amp_function
def fast_quantile(x, quant=0.95):
    """utils.py:84-102 for a float32 device tensor: the lower edge of the 10000-bin histogram bin at which the bins above bin 0 reach
    ``quant`` of their elements.  One extrema pass and one histogram pass on the device (``ops.histogram``: torch.histogram's CPU
    counts, exactly), then the walk on the host.  Returns a 0-dim float32 CPU tensor.
    Departure: the counts are exact integers; torch.histogram accumulates them in fp32, so a bin beyond 2^24 elements is inexact in
    the reference (the walk here still runs on the counts rounded to fp32 once)."""
    counts, edges = ops.histogram(x, QUANTILE_BINS)
    return quantile_walk(counts.cpu(), edges, quant)


def crop_offsets(full, crop):
    """(start, stop) of the reference's centre crop of ``crop`` out of ``full`` positions: floor(full/2) - floor(crop/2) to
    floor(full/2) + ceil(crop/2) -- correct for odd and even sizes on both sides."""
    c = full // 2
    start, stop = c - crop // 2, c + (crop + 1) // 2
    if crop < 0 or start < 0 or stop > full:
        raise ValueError(f"crop_volume_center: cannot crop {crop} out of {full}")
    return start, stop


def crop_volume_center(volume, volume_shape):
    """utils.py:105-126: the centre crop of the last two axes of a [N,D,H0,W0] tensor to ``volume_shape[2:4]``, as a view."""
    (h0, h1), (w0, w1) = crop_offsets(volume.shape[2], int(volume_shape[2])), crop_offsets(volume.shape[3], int(volume_shape[3]))
    return volume[:, :, h0:h1, w0:w1]


def _process_volume(vol, volume_new_size, volume_ths, norm, resize, out_dtype):
    if resize:
        raise NotImplementedError("load_process_volume: resize=True is not supported (the reference calls a resize_volume it does not define)")
    if norm == "std":
        raise NotImplementedError("load_process_volume: norm='std' is not supported")
    if norm is not None and norm != "max":
        raise ValueError(f"load_process_volume: unknown norm {norm!r}")       # the reference leaves out_volume unbound here
    if vol.dim() != 4:
        raise ValueError(f"load_process_volume: expected [D,H,W] or [N,D,H,W], got {tuple(vol.shape)}")
    H, W = int(volume_new_size[0]), int(volume_new_size[1])
    (oh, _), (ow, _) = crop_offsets(vol.shape[2], H), crop_offsets(vol.shape[3], W)
    args = dict(size=(H, W), offsets=(oh, ow), out_dtype=out_dtype)
    if norm == "max":
        if isinstance(volume_ths, (list, tuple)):
            raise TypeError("load_process_volume: norm='max' compares with a scalar volume_ths")
        # the reference compares the fp16 quotients with the scalar in fp16: the threshold is rounded to fp16 first
        return ops.prep_volumes(vol, mode="maxnorm", t0=float(torch.tensor(float(volume_ths), dtype=torch.float16)), **args)[0]
    if isinstance(volume_ths, float):
        mx = ops.prep_volumes(vol, mode="max_only", **args)[1].cpu()[0]
        return ops.prep_volumes(vol, mode="le", t0=float(volume_ths * mx), **args)[0]     # the product in fp32, as there
    if len(volume_ths) == 2:
        t1 = float(torch.tensor(float(volume_ths[1]), dtype=torch.float16))                # stored into the fp16 tensor
        return ops.prep_volumes(vol, mode="two", t0=ops._f32(volume_ths[0]), t1=t1, **args)[0]
    return ops.prep_volumes(vol, mode="none", **args)[0]


def _as_volumes(data_path, channel_order):
    if isinstance(data_path, str):
        raise NotImplementedError("load_process_volume: reading a file is the reference's; pass the fp16 tensor")
    if not torch.is_tensor(data_path) or data_path.dtype != torch.float16:
        raise TypeError("load_process_volume: expected a float16 tensor (the storage type of XLFMDatasetFull.vols)")
    vol = data_path
    if vol.dim() == 3:
        if channel_order == "xyz":
            vol = vol.permute(2, 1, 0)
        if channel_order == "yxz":
            vol = vol.permute(2, 0, 1)
        vol = vol.unsqueeze(0)
    return vol


@amp_region
def load_process_volume(data_path, volume_new_size=[], volume_ths=[], norm="max", resize=False, channel_order="zxy", device="cpu"):
    """utils.py:128-184 for an fp16 device tensor [D,H,W] or [N,D,H,W], same signature (``device`` is ignored: the tensor stays where
    it is): the centre crop to ``volume_new_size[0] x volume_new_size[1]`` and the threshold / normalisation step, one fused kernel
    (plus one maximum pass where the step needs the maximum).  Returns fp16 like the reference, bit-equal.
    ``norm='std'``, ``resize=True`` and file paths raise NotImplementedError."""
    return _process_volume(_as_volumes(data_path, channel_order), volume_new_size, volume_ths, norm, resize, torch.float16)


@amp_region
def prepare_XLFM_data(ds, vol_shape, volume_ths, volume_quantiles, img_ths, norm):
    """The body of load_XLFM_data (utils.py:208-220) behind the dataset object: ``ds`` is any object with ``.vols`` (fp16 [N,D,H0,W0]) and
    ``.stacked_views`` on the HIP device.  In the reference's order: crop + threshold of the volumes (widened to fp32 by the same
    kernel), the clamp of the volumes at the ``volume_quantiles[1]`` quantile, the image threshold at ``max * img_ths[0]``.
    Returns ``ds``."""
    ds.vols = _process_volume(_as_volumes(ds.vols, "zxy"), vol_shape, volume_ths, norm, False, torch.float32)
    ds.stacked_views = ds.stacked_views.float()
    if volume_quantiles[1] != 1:
        upper = fast_quantile(ds.vols, volume_quantiles[1])
        ops.prep_apply(ds.vols, "clamp_zero", a=upper, lower=False)
    views = ds.stacked_views if ds.stacked_views.is_contiguous() else ds.stacked_views.contiguous()
    img_low = ops.volume_extrema(views.reshape(1, 1, 1, -1))[0, 1].cpu() * img_ths[0]       # fp32 scalar product, as there
    ds.stacked_views = ops.prep_apply(views, "clamp_zero", b=img_low, upper=False)
    return ds
