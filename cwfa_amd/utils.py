"""Evaluation helpers (reference: utils.py): ``psnr`` (:380-394), ``volume_2_projections`` (:281-327), ``norm_data`` /
``filter_data`` (:419-446), and the data preparation in front of a run: ``fast_quantile`` (:84-102), ``crop_volume_center``
(:105-126), ``load_process_volume`` (:128-184) and ``prepare_XLFM_data``, the body of ``load_XLFM_data`` (:187-220) behind the
dataset object.  The passes over volumes are HIP kernels (csrc/eval_ops.hip, csrc/prep_ops.hip); no torch operator runs on a volume.

``cwfa_amd.install()`` does NOT register this module as ``utils`` (the reference's ``utils`` also holds its dataset loaders);
``cwfa_amd.install(utils=True)`` does, for the ``from utils import *`` of ``main_deconvolve_dataset.py``.
Inputs are assumed finite (the kernels do not propagate NaN)."""
import numpy as np
import torch

from . import _lib, ops
from .amp import amp_function, amp_region

__all__ = ["psnr", "volume_2_projections", "norm_data", "filter_data", "fast_quantile", "crop_volume_center", "load_process_volume",
           "prepare_XLFM_data", "roll_n", "batch_fftshift2d_real", "fft_conv", "fft_conv_split", "load_PSF", "load_PSF_OTF",
           "XLFMDeconv", "XLFMForward", "simulate_XLFM_image"]


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


# ------------------------------------------------------------------------------------------------ Richardson-Lucy deconvolution
def roll_n(X, axis, n):
    """utils.py:451-463: X rolled along ``axis`` so that element n comes first (``torch.roll`` by -n); a torch operator, the
    deconvolution itself does not go through it."""
    return torch.roll(X, -int(n), axis)


def batch_fftshift2d_real(x):
    """utils.py:465-477 for a real float32 device tensor [B, C, H, W]: every plane rolled by ceil(size / 2) along both axes (the
    source index is the target index plus the shift) -- one launch of the projection kernel with one depth per plane."""
    if torch.is_tensor(x) and x.is_complex():
        raise TypeError("batch_fftshift2d_real: real tensors only")
    ops._dev(x, "x")
    if x.dim() != 4:
        raise ValueError(f"batch_fftshift2d_real: expected [B,C,H,W], got {tuple(x.shape)}")
    B, Cc, H, W = x.shape
    x = x if x.is_contiguous() else x.contiguous()
    return ops.deconv_project(x.view(B * Cc, 1, H, W)).view(B, Cc, H, W)


def _full_size(fullSize, what):
    fh, fw = (int(v) for v in fullSize)
    if fw % 2:
        raise ValueError(f"{what}: the full width {fw} is odd: the reference's irfft2 returns {fw - 1} columns and its result is short")
    return fh, fw


def _pad_centre(A, fh, fw, what):
    """F.pad of utils.py:492-498: ceil(d / 2) zeros in front and floor(d / 2) behind, on both axes."""
    dh, dw = fh - A.shape[2], fw - A.shape[3]
    if dh < 0 or dw < 0:
        raise ValueError(f"{what}: a {A.shape[2]} x {A.shape[3]} plane does not fit the full size {fh} x {fw}")
    return torch.nn.functional.pad(A, [(dw + 1) // 2, dw // 2, (dh + 1) // 2, dh // 2])


def _conv_spectrum(A, B, fh, fw, B_precomputed, what):
    """irfft2(rfft2(pad(A)) * OTF) of utils.py:498-510, unshifted: (real planes [Ba, n, fh, fw], OTF [1, n, fh, fw // 2 + 1])."""
    ops._dev(A, "A")
    if A.dim() != 4:
        raise ValueError(f"{what}: expected [B,n,H,W], got {tuple(A.shape)}")
    if B_precomputed:
        otf = ops._cdev(B.detach(), "B")
    else:
        ops._dev(B, "B")
        otf = torch.fft.rfft2(_pad_centre(B.detach(), fh, fw, what))
    if otf.dim() != 4 or otf.shape[0] != 1 or tuple(otf.shape[1:]) != (A.shape[1], fh, fw // 2 + 1):
        raise ValueError(f"{what}: the transfer function {tuple(otf.shape)} does not fit {A.shape[1]} planes of {fh} x {fw}")
    spec = torch.fft.rfft2(_pad_centre(A, fh, fw, what))
    for b in range(spec.shape[0]):
        ops.deconv_spectrum_mul(spec[b], otf[0], out=spec[b])
    return torch.fft.irfft2(spec, s=(fh, fw)), otf


def fft_conv(A, B, fullSize, Bshape=[], B_precomputed=False):
    """utils.py:480-510, same signature and both return forms: the shifted planes of irfft2(rfft2(pad A) * OTF), and the OTF too
    when it is computed here (``B`` a PSF [1, n, h, w]) rather than given (``B_precomputed``).  float32 device tensors.
    An odd full width raises ValueError (the reference's result comes out one column short)."""
    fh, fw = _full_size(fullSize, "fft_conv")
    real, otf = _conv_spectrum(A, B, fh, fw, B_precomputed, "fft_conv")
    out = batch_fftshift2d_real(real)
    return out if B_precomputed else (out, otf)


def fft_conv_split(A, B, psf_shape, n_split, B_precomputed=False, device="cuda"):
    """utils.py:513-550, same signature (``device`` is ignored: the tensors stay where they are): the image of a volume
    A [Ba, D, h, w] under the PSF / OTF B, cropped to ``psf_shape``, in ``n_split`` depth chunks, |chunk sum| added per chunk.
    Shift, crop, depth sum and abs are one kernel per chunk.  Returns the image [Ba, 1, psf, psf], and the OTF
    [1, D, full_h, full_w // 2 + 1] when it is computed here.  As in the reference the chunks hold D // n_split depths and only
    the first n_split chunks are used."""
    if A.dim() != 4:
        raise ValueError(f"fft_conv_split: expected [B,D,H,W], got {tuple(A.shape)}")
    D = A.shape[1]
    ph, pw = (int(v) for v in psf_shape)
    n_split = int(n_split)
    if n_split < 1 or n_split > D:
        raise ValueError(f"fft_conv_split: n_split = {n_split} does not divide {D} depths into chunks")
    fh, fw = _full_size((A.shape[2] + ph, A.shape[3] + pw), "fft_conv_split")
    ops._dev(A, "A")
    step = D // n_split
    oy, ox = -((ph - fh) // 2), -((pw - fw) // 2)
    img = torch.zeros(A.shape[0], 1, ph, pw, dtype=torch.float32, device=A.device)
    otf_out = None if B_precomputed else torch.zeros(1, D, fh, fw // 2 + 1, dtype=torch.complex64, device=A.device)
    for n in range(n_split):
        sl = slice(n * step, (n + 1) * step)
        real, otf = _conv_spectrum(A[:, sl], B[:, sl].contiguous(), fh, fw, B_precomputed, "fft_conv_split")
        if not B_precomputed:
            otf_out[:, sl] = otf
        ops.deconv_project(real, out=img, window=(oy, ox, ph, pw), post="abs", accumulate=True)
    return img if B_precomputed else (img, otf_out)


def load_PSF(psf, depths_to_use=[], interleaved=True):
    """utils.py:553-591 behind the file reading: ``psf`` is the tensor [1, D, H, W] the reference builds from the file.  Made square
    (``pad_img_to_min``), the depths chosen (an int n: n interleaved depths, or the n central ones; -1: all; a list: those), every
    depth divided by its sum.  Torch operators: this runs once per PSF."""
    from .XLFMDataset import pad_img_to_min
    if isinstance(psf, str):
        raise NotImplementedError("load_PSF: reading a file is the reference's; pass the PSF tensor [1, D, H, W]")
    psfIn = pad_img_to_min(psf)
    if isinstance(depths_to_use, int):
        if depths_to_use == -1:
            depths_to_use = list(range(psfIn.shape[1]))
        else:
            n_depths = depths_to_use
            if interleaved:
                depths_to_use = torch.linspace(0, psfIn.shape[1], n_depths + 2).long()[1:-1]
            else:
                first = psfIn.shape[1] // 2 - n_depths // 2 + 1
                depths_to_use = list(range(first, first + n_depths))
    psfIn = psfIn[:, depths_to_use, ...]                                  # advanced indexing: a copy, as there
    return psfIn / psfIn.sum((2, 3), keepdim=True)


def load_PSF_OTF(psf, vol_size, n_split=20, downS=1, device="cuda", dark_current=106, calc_max=False, compute_OTF=False):
    """utils.py:593-627 for a PSF tensor on the HIP device: (OTF, psf_shape) with OTF complex64 [1, D, full, full // 2 + 1] for a
    volume of ``vol_size`` = [h, w, D], or [.., 2] with the conjugate behind it for ``compute_OTF``.  ``calc_max`` raises
    NotImplementedError (the reference returns a name it never defines)."""
    if calc_max:
        raise NotImplementedError("load_PSF_OTF: calc_max=True is not supported (the reference fails there on an undefined name)")
    n_depths = int(vol_size[-1])
    if n_split == -1:
        n_split = n_depths
    psfIn = load_PSF(psf, n_depths).float()
    psf_shape = torch.tensor(psfIn.shape[2:])
    vol = torch.zeros(1, psfIn.shape[1], int(vol_size[0]), int(vol_size[1]), dtype=torch.float32, device=psfIn.device)
    OTF = fft_conv_split(vol, psfIn.contiguous(), psf_shape, n_split=n_split)[1]       # the reference's random volume only sizes it
    if compute_OTF:
        OTF = torch.stack((OTF, OTF.conj().resolve_conj()), 4)
    return OTF, psf_shape


MAP_PRIOR_BOUND = 2.0 ** 60      # XLFMDeconv refuses a prior whose w or w |mean| lies above it (the fp32 M-step would overflow)


def _deconv_sizes(OTF, img, ObjSize):
    """The shapes XLFMDeconv can run (the reference's pads come out short on the others), or ValueError naming the size."""
    F = int(OTF.shape[2])
    if F % 2:
        raise ValueError(f"XLFMDeconv: the full size {F} is odd: irfft2 returns {F - 1} columns")
    if OTF.shape[3] != F // 2 + 1:
        raise ValueError(f"XLFMDeconv: the OTF's last axis is {OTF.shape[3]}, a square full size {F} needs {F // 2 + 1}")
    obj = int(ObjSize[0])
    if int(ObjSize[1]) != obj:
        raise ValueError(f"XLFMDeconv: the object {list(ObjSize)} is not square")
    if obj > F or (F - obj) % 2:
        raise ValueError(f"XLFMDeconv: the object size {obj} cannot be padded evenly to the full size {F}")
    if img.dim() != 4 or img.shape[0] != 1 or img.shape[1] != 1:
        raise ValueError(f"XLFMDeconv: expected one image [1,1,H,W], got {tuple(img.shape)}")
    ih = int(img.shape[2])
    if int(img.shape[3]) != ih:
        raise ValueError(f"XLFMDeconv: the image {ih} x {int(img.shape[3])} is not square")
    if ih > F or (F - ih) % 2:
        raise ValueError(f"XLFMDeconv: the image size {ih} cannot be padded evenly to the full size {F}")
    return F, obj, (F - obj) // 2, (F - ih) // 2


def XLFMDeconv(OTF, img, nIt, ObjSize=[512, 512], PSFShape=[2160, 2160], ROIsize=[512, 512, 90], errorMetric=torch.nn.functional.mse_loss,
               n_split_fourier=1,
               update_median_limit_multiplier=10, max_allowed=4500, device="cuda:0", all_in_device=False, verbose=False, *,
               accelerate=False, alpha_max=0.999, trace=False, tol=None, check_every=5, prior_mean=None, prior_std=None, prior_weight=1.0,
               init=None):
    """Richardson-Lucy deconvolution of one image; utils.py:630-738, same signature and return forms.

    OTF: complex64 [1, D, F, F // 2 + 1] (the conjugate is applied on the fly) or [1, D, F, F // 2 + 1, 2] (``OTF[..., 1]`` is used
    for the back projection as given); img float32 [1, 1, H, W]; all on the HIP device, all results stay there.  Returns
    (ObjRecon [1, D, obj, obj], 0, ImgEst [1, 1, F, F], [], padSize, padSizeImg); an image that sums to zero returns
    (zeros, their composite projection on the CPU, img, []).  ``n_split_fourier`` depths go through the FFTs at a time (1: all).
    Per iteration and chunk: rfft2 of the padded object, spectrum product, irfft2, shift + relu + depth sum (forward); ratio, median
    of the non-zero elements, clamp; rfft2 of the ratio, product with the conjugate OTF, irfft2, shifted product into the object's
    window (backward).  The object stays zero-padded throughout, every buffer is allocated before the loop.  A non-finite image
    pixel makes the ratio NaN in the first iteration and stops the loop there, as the reference's ``0 * ImgExp`` start does.
    ``device``, ``all_in_device``, ``errorMetric`` and ``max_allowed`` are accepted and unused; ``verbose`` raises
    NotImplementedError (it plots).  img and OTF are left unchanged.

    Beyond the reference, all off by default (the default call issues the launches and returns the bits it always did):
    ``accelerate``: Biggs-Andrews vector extrapolation.  The padded object holds a prediction y_k, the
    iteration above is applied to it (x_{k+1}), the step g_k = x_{k+1} - y_k gives alpha = sum(g_k g_{k-1}) / sum(g_{k-1}^2) in
    float64 over the whole window, clamped to [0, ``alpha_max``] (0 without a previous step or a finite quotient), and
    y_{k+1} = max(x_{k+1} + alpha (x_{k+1} - x_k), 0).  Two more streaming passes over the window per iteration, no FFT; alpha never
    leaves the device.  The volume returned is the last x, ImgEst the projection of the last y.
    ``trace``: the fourth slot holds the Poisson negative log-likelihood sum(est - img log(est + 1e-8)) of every iteration run, as
    Python floats (float64 on the device, copied once after the loop).
    ``tol``: every ``check_every`` iterations the likelihood is read; when (previous checked - this) / |this| < tol the iteration
    is completed and the loop ends.
    ``prior_mean``, ``prior_std`` (both or neither; float32 [1, D, obj, obj] on the device, e.g. from ``prior_from_posterior``),
    ``prior_weight`` >= 0: MAP Richardson-Lucy under an independent Gaussian prior N(prior_mean, prior_std^2) per voxel (DESIGN.md
    section 21).  With a the plain update of a voxel and w = prior_weight / prior_std^2 (formed once, in fp32), the new value is
    the maximiser of -x + a log x - w / 2 (x - mean)^2: c = 1 - w mean, r = sqrt(c^2 + 4 w a), x = 2a / (c + r) where c > 0 and
    (r - c) / (2w) elsewhere.  ``prior_std = inf`` is "no prior here", w = 0 everywhere returns the plain call's bits; the mean may
    be negative.  Works with ``accelerate`` (x_{k+1} is the MAP update of y_k).  ValueError, once before the loop, for a std that is
    not > 0 (NaN included), a mean that is not finite, and w or w |mean| above 2^60 (then c^2 <= 2^121 and 2w <= 2^61 are finite
    in fp32, and 4 w a is for every a below 2^64; a std of 1e-9 at weight 1 is still inside).  With a prior, ``trace`` and ``tol``
    see the objective: the likelihood plus sum(w / 2 (y_k - mean)^2) of the point y_k that was projected, in float64; it is complete
    once the iteration's update has run, so that is where ``tol`` reads it.
    ``init``: float32 [1, D, obj, obj] on the device, finite and >= 0: the start object in place of the ones (x_0 = y_0 = init with
    ``accelerate``); usable without a prior.  A voxel that starts at 0 stays 0 without a prior."""
    if verbose:
        raise NotImplementedError("XLFMDeconv: verbose=True plots every iteration with matplotlib; not supported")
    if not 0.0 <= float(alpha_max) < 1.0:
        raise ValueError(f"XLFMDeconv: alpha_max = {alpha_max} is not in [0, 1)")
    if tol is not None and not float(tol) > 0.0:
        raise ValueError(f"XLFMDeconv: tol = {tol} is not positive")
    if int(check_every) < 1:
        raise ValueError(f"XLFMDeconv: check_every = {check_every} is below 1")
    if not torch.is_tensor(OTF) or OTF.dim() not in (4, 5) or (OTF.dim() == 5 and OTF.shape[4] != 2) or OTF.shape[0] != 1:
        raise ValueError("XLFMDeconv: the OTF must be [1, D, F, F // 2 + 1] or [1, D, F, F // 2 + 1, 2]")
    nDepths = int(OTF.shape[1])
    step = nDepths if n_split_fourier == 1 else int(n_split_fourier)
    if step < 1:
        raise ValueError(f"XLFMDeconv: n_split_fourier = {n_split_fourier}")
    F, obj, po, pi = _deconv_sizes(OTF, img, ObjSize)
    if (prior_mean is None) != (prior_std is None):
        raise ValueError("XLFMDeconv: prior_mean and prior_std are given together or not at all")
    if not float(prior_weight) >= 0.0 or float(prior_weight) == float("inf"):
        raise ValueError(f"XLFMDeconv: prior_weight = {prior_weight} is not a finite number >= 0")
    for name, t in (("prior_mean", prior_mean), ("prior_std", prior_std), ("init", init)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (1, nDepths, obj, obj)):
            raise ValueError(f"XLFMDeconv: {name} must be a float32 tensor [1, {nDepths}, {obj}, {obj}], got "
                             f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t)}")
    ops._dev(img, "img")
    dev = img.device
    prior = prior_mean is not None
    for name, t in (("prior_mean", prior_mean), ("prior_std", prior_std), ("init", init)):
        if t is not None and ops._dev(t, name).device != dev:
            raise ValueError(f"XLFMDeconv: {name} is on {t.device}, the image on {dev}")
    if prior or init is not None:                                          # one read-back for every refusal, before the loop
        with torch.no_grad():
            bad = []
            if prior:
                mu, std = prior_mean.contiguous(), prior_std.contiguous()
                w_map = float(prior_weight) / (std * std)
                bad += [~(std > 0), ~torch.isfinite(mu), ~(w_map <= MAP_PRIOR_BOUND), ~(w_map * mu.abs() <= MAP_PRIOR_BOUND)]
            if init is not None:
                bad += [~torch.isfinite(init) | ~(init >= 0)]
            bad = torch.stack([b.any() for b in bad]).tolist()
        reasons = (["prior_std is not > 0 everywhere (NaN included; +inf switches the prior off)", "prior_mean is not finite everywhere",
                    "prior_weight / prior_std^2 exceeds 2^60", "prior_weight / prior_std^2 * |prior_mean| exceeds 2^60"] if prior else []) + \
                  (["init is not finite and >= 0 everywhere"] if init is not None else [])
        for flag_, reason in zip(bad, reasons):
            if flag_:
                raise ValueError(f"XLFMDeconv: {reason}")
    if float(img.sum()) == 0:
        volOut = torch.zeros(img.shape[0], nDepths, obj, obj, dtype=torch.float32, device=dev)
        return volOut, volume_2_projections(volOut.permute(0, 2, 3, 1).unsqueeze(1)), img, []
    if OTF.dim() == 5:                                                     # the reference clones both halves too
        otf_f, otf_b, conj = OTF[..., 0].contiguous(), OTF[..., 1].contiguous(), False
    else:
        otf_f = otf_b = OTF if OTF.is_contiguous() else OTF.contiguous()
        conj = True
    ops._cdev(otf_f, "OTF")
    padSize, padSizeImg = 2 * [po] + 2 * [po], 2 * [pi] + 2 * [pi]
    Fh = F // 2 + 1
    with torch.no_grad():
        ImgExp = torch.nn.functional.pad(img, padSizeImg).contiguous()
        obj_pad = torch.zeros(1, nDepths, F, F, dtype=torch.float32, device=dev)
        obj_pad[:, :, po:po + obj, po:po + obj] = 1.0 if init is None else init
        spec = torch.empty(1, min(step, nDepths), F, Fh, dtype=torch.complex64, device=dev)
        real = torch.empty(1, min(step, nDepths), F, F, dtype=torch.float32, device=dev)
        rspec = torch.empty(1, 1, F, Fh, dtype=torch.complex64, device=dev)
        ImgEst = torch.zeros(1, 1, F, F, dtype=torch.float32, device=dev)
        Tmp = torch.empty_like(ImgEst)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        median = (torch.empty(1, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int64, device=dev))
        ws = torch.empty(_lib.SELECT_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
        chunks = [(jj, min(jj + step, nDepths)) for jj in range(0, nDepths, step)]
        nIt, done, stop, checked = int(nIt), 0, False, None
        if accelerate:                                                     # x_k (ones), x_{k+1}, g_{k-1} (none: zeros), the sums, alpha
            x_prev = torch.ones(1, nDepths, obj, obj, dtype=torch.float32, device=dev) if init is None else init.clone().contiguous()
            x_new, g = torch.empty_like(x_prev), torch.zeros_like(x_prev)
            slab = ops.deconv_accel_slab(min(step, nDepths), obj, dev)
            alpha = torch.zeros(1, dtype=torch.float32, device=dev)
        if trace or tol is not None:
            nll = torch.zeros(max(nIt, 1), dtype=torch.float64, device=dev)
            nll_ws = torch.empty(_lib.DECONV_NLL_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
        # with a prior the trace holds the objective: the update kernels add the penalty of what they read to a slab of its own
        pen = ops.deconv_penalty_slab(min(step, nDepths), obj, dev) if prior and (trace or tol is not None) else None
        for ii in range(nIt):
            for jj, je in chunks:                                          # forward projection
                sp, re = spec[:, :je - jj], real[:, :je - jj]
                torch.fft.rfft2(obj_pad[:, jj:je], out=sp)
                ops.deconv_spectrum_mul(sp, otf_f[:, jj:je], out=sp)
                torch.fft.irfft2(sp, s=(F, F), out=re)
                ops.deconv_project(re, out=ImgEst, pre="relu", accumulate=jj > 0)
            ops.deconv_ratio(ImgExp, ImgEst, Tmp, flag)
            ops.select_nonzero(Tmp, out=median, workspace=ws)
            ops.deconv_clamp(Tmp, median[0], median[1], update_median_limit_multiplier)
            if trace or tol is not None:
                ops.deconv_poisson_nll(ImgExp, ImgEst, nll, ii, nll_ws)
            if int(flag.item()):
                print(F'nan found at it: {ii+1} ')
                ImgEst += 0 * ImgExp                                       # the NaN the reference's estimate carries from its start
                break
            if tol is not None and pen is None and (ii + 1) % int(check_every) == 0:
                now = float(nll[ii].item())
                stop = checked is not None and (checked - now) / abs(now) < float(tol)
                checked = now
            torch.fft.rfft2(Tmp, out=rspec)
            for jj, je in chunks:                                          # back projection and update
                sp, re = spec[:, :je - jj], real[:, :je - jj]
                ops.deconv_spectrum_mul(rspec, otf_b[:, jj:je], conj=conj, out=sp)
                torch.fft.irfft2(sp, s=(F, F), out=re)
                if prior and accelerate:
                    ops.deconv_update_accel_map(obj_pad[:, jj:je], re, g[:, jj:je], x_new[:, jj:je], mu[:, jj:je], w_map[:, jj:je], slab, obj,
                                                po, pen)
                elif prior:
                    ops.deconv_update_map(obj_pad[:, jj:je], re, mu[:, jj:je], w_map[:, jj:je], obj, po, pen)
                elif accelerate:
                    ops.deconv_update_accel(obj_pad[:, jj:je], re, g[:, jj:je], x_new[:, jj:je], slab, obj, po)
                else:
                    ops.deconv_update(obj_pad[:, jj:je], re, obj, po)
            if pen is not None:                                            # the objective of y_k is complete only now
                ops.deconv_penalty(pen, nll, ii)
                if tol is not None and (ii + 1) % int(check_every) == 0:
                    now = float(nll[ii].item())
                    stop = checked is not None and (checked - now) / abs(now) < float(tol)
                    checked = now
            done = ii + 1
            if accelerate:
                ops.deconv_alpha(slab, alpha_max, alpha)
                if done < nIt and not stop:
                    ops.deconv_predict(obj_pad, x_new, x_prev, alpha, obj, po)
                x_new, x_prev = x_prev, x_new                              # x_prev is the latest iterate from here on
            if stop:
                break
        ObjRecon = x_prev if accelerate else obj_pad[:, :, po:po + obj, po:po + obj].contiguous()
        losses = nll[:done].tolist() if trace else []
    ObjRecon[:, 0:nDepths // 2 - ROIsize[2] // 2, ...] = 0
    ObjRecon[:, nDepths // 2 + ROIsize[2] // 2:, ...] = 0
    return ObjRecon, 0, ImgEst, losses, padSize, padSizeImg


def prior_from_posterior(mean, std, n_depths, obj_size, scale=1.0, offset=0.0):
    """(prior_mean, prior_std) for ``XLFMDeconv``: the flow's per-voxel posterior moments [1, d, h, w] (``CWFA.posterior_moments``)
    centre-embedded into [1, n_depths, obj_size, obj_size].  Inside: ``mean * scale + offset`` and ``std * scale``; outside: mean 0 and
    std +inf, "no prior here".  The embedding uses ``crop_offsets`` on the three axes, so with scale 1 and offset 0
    ``crop_volume_center`` of either result (and the same centre crop of its depths) gives the input back bit for bit.  Plain torch, on
    whatever device the moments are on.
    Units: ``posterior_moments(std_scale=...)`` and ``denormalise_prediction`` bring the moments back to the dataset's volume units
    (a de-normalised mean may be negative, which the deconvolution accepts); any further factor between the dataset's normalisation
    and the photon units the deconvolution's volume is in is the caller's ``scale``."""
    if not torch.is_tensor(mean) or not torch.is_tensor(std) or mean.dim() != 4 or mean.shape[0] != 1 or tuple(mean.shape) != tuple(std.shape):
        raise ValueError("prior_from_posterior: mean and std must be two [1, d, h, w] tensors of one shape")
    n_depths, obj_size = int(n_depths), int(obj_size)
    (d0, d1), (h0, h1), (w0, w1) = (crop_offsets(full, int(crop)) for full, crop in zip((n_depths, obj_size, obj_size), mean.shape[1:]))
    prior_mean = torch.zeros(1, n_depths, obj_size, obj_size, dtype=mean.dtype, device=mean.device)
    prior_std = torch.full_like(prior_mean, float("inf"))
    neutral = float(scale) == 1.0 and float(offset) == 0.0
    prior_mean[:, d0:d1, h0:h1, w0:w1] = mean if neutral else mean * scale + offset
    prior_std[:, d0:d1, h0:h1, w0:w1] = std if neutral else std * scale
    return prior_mean, prior_std


def XLFMForward(OTF, vol, ObjSize=None, img_size=None, n_split_fourier=1, out=None):
    """The forward projection of ``XLFMDeconv``'s loop on its own: the image a volume gives under the transfer function.

    OTF as for ``XLFMDeconv`` (the 5-D form uses ``OTF[..., 0]``); vol float32 [1, D, obj, obj] on the HIP device (``ObjSize``, if
    given, must name that size).  Returns the estimate [1, 1, F, F], or with ``img_size`` its centred [1, 1, img_size, img_size]
    window (the bits of that window of the full result: the depth sum reads the window only).  Per chunk of ``n_split_fourier``
    depths (1: all) the launches are those of the loop: rfft2 of the zero-padded chunk, ``deconv_spectrum_mul``, irfft2,
    ``deconv_project(pre="relu")`` with the shift and the depth sum.  ``out``: a contiguous float32 tensor of the result's size to
    write into.  vol and OTF are left unchanged."""
    if not torch.is_tensor(OTF) or OTF.dim() not in (4, 5) or (OTF.dim() == 5 and OTF.shape[4] != 2) or OTF.shape[0] != 1:
        raise ValueError("XLFMForward: the OTF must be [1, D, F, F // 2 + 1] or [1, D, F, F // 2 + 1, 2]")
    nDepths = int(OTF.shape[1])
    step = nDepths if n_split_fourier == 1 else int(n_split_fourier)
    if step < 1:
        raise ValueError(f"XLFMForward: n_split_fourier = {n_split_fourier}")
    ops._dev(vol, "vol")
    if vol.dim() != 4 or vol.shape[0] != 1 or vol.shape[1] != nDepths or vol.shape[2] != vol.shape[3]:
        raise ValueError(f"XLFMForward: expected a volume [1, {nDepths}, obj, obj], got {tuple(vol.shape)}")
    obj = int(vol.shape[2])
    if ObjSize is not None and [int(v) for v in ObjSize[:2]] != [obj, obj]:
        raise ValueError(f"XLFMForward: ObjSize {list(ObjSize)} is not the volume's {obj} x {obj}")
    F = int(OTF.shape[2])
    if F % 2 or OTF.shape[3] != F // 2 + 1:
        raise ValueError(f"XLFMForward: the OTF's planes {tuple(OTF.shape[2:4])} are not [F, F // 2 + 1] of an even full size F")
    if obj > F or (F - obj) % 2:
        raise ValueError(f"XLFMForward: the object size {obj} cannot be padded evenly to the full size {F}")
    size = F if img_size is None else int(img_size[0] if isinstance(img_size, (list, tuple)) else img_size)
    if isinstance(img_size, (list, tuple)) and int(img_size[-1]) != size:
        raise ValueError(f"XLFMForward: the image {list(img_size)} is not square")
    if size < 1 or size > F or (F - size) % 2:
        raise ValueError(f"XLFMForward: the image size {size} is not a centred window of the full size {F}")
    po, pi = (F - obj) // 2, (F - size) // 2
    otf_f = OTF[..., 0] if OTF.dim() == 5 else OTF
    otf_f = ops._cdev(otf_f if otf_f.is_contiguous() else otf_f.contiguous(), "OTF")
    dev = vol.device
    with torch.no_grad():
        if out is None:
            out = torch.empty(1, 1, size, size, dtype=torch.float32, device=dev)
        nz = min(step, nDepths)
        obj_pad = torch.zeros(1, nz, F, F, dtype=torch.float32, device=dev)
        spec = torch.empty(1, nz, F, F // 2 + 1, dtype=torch.complex64, device=dev)
        real = torch.empty(1, nz, F, F, dtype=torch.float32, device=dev)
        window = None if size == F else (pi, pi, size, size)
        for jj in range(0, nDepths, step):
            je = min(jj + step, nDepths)
            pad, sp, re = obj_pad[:, :je - jj], spec[:, :je - jj], real[:, :je - jj]
            pad[:, :, po:po + obj, po:po + obj] = vol[:, jj:je]
            torch.fft.rfft2(pad, out=sp)
            ops.deconv_spectrum_mul(sp, otf_f[:, jj:je], out=sp)
            torch.fft.irfft2(sp, s=(F, F), out=re)
            ops.deconv_project(re, out=out, window=window, pre="relu", accumulate=jj > 0)
    return out


def simulate_XLFM_image(OTF, vol, photons=None, background=0.0, seed=0, sample_offset=0, n_samples=1, **forward_kw):
    """(clean [1, 1, S, S], noisy [n_samples, 1, S, S]): a measurement of a volume.  clean = ``XLFMForward(OTF, vol, **forward_kw)``;
    the noisy images are Poisson draws, in photon units, at the fp32 rate  clean * (photons / max(clean)) + background  (``photons`` at
    the brightest pixel; None: the clean image is in photon units already, rate = clean + background).  The maximum is taken on the
    device (``ops.volume_extrema``) and nothing is read back; an all-zero clean image with ``photons`` gives NaN rates, hence NaN.
    Sample s is ``ops.rand_poisson`` sample ``sample_offset + s`` of stream 0 under ``seed``: ``n_samples = 3`` equals three calls
    with ``sample_offset`` 0, 1 and 2."""
    clean = XLFMForward(OTF, vol, **forward_kw)
    with torch.no_grad():
        rate = clean[0]                                                    # [1, S, S]: one plane shared by all samples
        if photons is not None:
            rate = rate * (float(photons) / ops.volume_extrema(clean.reshape(1, 1, 1, -1))[0, 1])
        if float(background) != 0.0:
            rate = rate + float(background)
        noisy = ops.rand_poisson(rate.contiguous(), seed, stream=0, sample_offset=sample_offset, n_samples=int(n_samples))
    return clean, noisy
