"""The pieces of the reference's XLFMDataset.py around the hot path: cropping the 29 lenslet views out of the sensor frame
(SURVEY.md section 8f, row 2), the clean-up and centre crop of the raw frames (XLFMDataset.py:15-40,101-104,160-162) and the
statistics / normalisation of ``ConcatDataset`` (:251-395) on device tensors, and the shot-noise augmentation
the reference documents (:397-405) but never defines per dataset.  File reading stays the
reference's.  Not registered by cwfa_amd.install(); a maintainer patches the calls, see INTEGRATION.md."""
import math
from collections import namedtuple

import torch

from . import ops
from .amp import amp_function, amp_region

__all__ = ["XLFMDatasetFull", "ConcatDataset", "extract_views", "pad_img_to_min", "center_crop", "prepare_frames", "shot_noise_scales", "add_random_shot_noise_to_datasets",
           "extract_sparse", "SparseSplit", "quantile_rank", "estimate_shifts", "shift_frames", "register_frames", "valid_window", "Registration",
           "view_labels", "estimate_view_shifts", "fit_view_shifts", "shift_views", "register_views", "valid_view_windows", "ViewFit", "ViewRegistration"]


def extract_views(image, lenslet_coords, subimage_shape, debug=False):
    """XLFMDatasetFull.extract_views, XLFMDataset.py:212-242 (same signature; ``debug`` draws markers in the reference and
    is not supported here)."""
    if debug:
        raise NotImplementedError("extract_views(debug=True) is a plotting aid of the reference")
    return ops.extract_views(image, lenslet_coords, subimage_shape)


def pad_amounts(h, w):
    """(rows, columns) ``pad_img_to_min`` takes off EACH side of an h x w image: it pads by the floor-halved negative difference to
    the shorter side, so it crops, and by one more than half where the difference is odd (the result is then one short)."""
    m = min(h, w)
    return -((m - h) // 2), -((m - w) // 2)


def pad_img_to_min(image):
    """XLFMDataset.py:15-25 as a view of the last two axes."""
    h, w = image.shape[-2:]
    ph, pw = pad_amounts(h, w)
    return image[..., ph:h - ph, pw:w - pw]


def center_crop(layer, target_size, pad=0):
    """XLFMDataset.py:27-40 for a [B,C,H,W] tensor, as a view."""
    dy, dx = (layer.shape[2] - target_size[0]) // 2 - pad, (layer.shape[3] - target_size[1]) // 2 - pad
    return layer[:, :, dy:dy + target_size[0], dx:dx + target_size[1]]


def frame_offsets(h, w, img_shape):
    """The index map of ``pad_img_to_min`` followed by ``center_crop``: output (r, c) is source (r + oy, c + ox).  Raises where the
    crop does not fit the padded image (the reference's slice comes out short and its store into ``stacked_views`` fails)."""
    ph, pw = pad_amounts(h, w)
    h1, w1 = h - 2 * ph, w - 2 * pw
    dy, dx = (h1 - int(img_shape[0])) // 2, (w1 - int(img_shape[1])) // 2
    if dy < 0 or dx < 0 or dy + img_shape[0] > h1 or dx + img_shape[1] > w1:
        raise ValueError(f"prepare_frames: a {img_shape[0]} x {img_shape[1]} crop does not fit the {h1} x {w1} image left of {h} x {w}")
    return ph + dy, pw + dx


@amp_function
def prepare_frames(raw, img_shape):
    """``stacked_views`` [N, img_shape[0], img_shape[1]] from raw fp32 frames [N,h,w] on the device, XLFMDataset.py:101-104,160-162 in
    one kernel: NaN -> 0, clip to [0, 50000], the round trip through fp16, ``pad_img_to_min`` and ``center_crop``."""
    return ops.prep_frames(raw, img_shape, frame_offsets(raw.shape[-2], raw.shape[-1], img_shape))


SparseSplit = namedtuple("SparseSplit", ["sparse", "baseline", "scales", "tau"])


def quantile_rank(q, n):
    """The 0-based rank of the ``q`` quantile of ``n`` samples by the rule of ``numpy.quantile(method="lower")``:
    floor(q * (n - 1)), formed in float64 on the host."""
    q, n = float(q), int(n)
    if not 0.0 <= q <= 1.0 or n < 1:
        raise ValueError(f"extract_sparse: a quantile in [0, 1] of at least one frame is expected, got q = {q}, N = {n}")
    return int(math.floor((n - 1) * q))


@amp_region
def extract_sparse(frames, baseline_q=0.5, noise_k=0.0, ths=0.0, scale="ls", pair=False, out=None):
    """The sparse (activity) component of a contiguous [N,H,W] fp32 / fp16 device stack under a robust rank-1 background
    L[t,p] = scales[t] * baseline[p] -- the classical form of the stage whose output the reference reads from
    ``SLNet_preprocessed/``; it is NOT SLNet's output.  Returns ``SparseSplit(sparse, baseline, scales, tau)``; nothing is read back
    to the host.

    A.  baseline[p]: the ``baseline_q`` quantile of pixel p over time (rank rule of ``numpy.quantile(method="lower")``).
        scales[t]:   ``scale="ls"``: the least-squares scale <frame t, baseline> / <baseline, baseline> from float64 dot products
                     (bleaching), 0 where the baseline is all zero; ``scale="none"``: ones.
    B.  only for ``noise_k != 0``: with m and lo the 0.5 and 0.1587 quantiles of the residual x - scales[t] * baseline[p] over time
        (its median and the point one sigma below it -- the lower half holds no transients),
        tau[p] = (m + noise_k * (m - lo)) + ths in fp32; otherwise tau is ``ths`` as a map, or None for ``ths == 0``.
    C.  sparse = relu(x - scales[t] * baseline[p] - tau[p]), float32 [N,H,W]; ``pair``: the reference's [N,H,W,2] layout with the
        frames in channel 0 and the sparse component in channel 1.  ``out``: where to write it (an fp32 ``frames`` itself: in place).
    Three reads of the stack, four with step B."""
    if not torch.is_tensor(frames) or frames.dim() != 3 or not frames.is_contiguous():
        raise ValueError("extract_sparse: a contiguous [N,H,W] stack is expected")
    if scale not in ("ls", "none"):
        raise ValueError(f"extract_sparse: scale is 'ls' or 'none', got {scale!r}")
    N = int(frames.shape[0])
    rank = quantile_rank(baseline_q, N)
    baseline = ops.temporal_select(frames, [rank])[0]
    if scale == "ls":
        sums = ops.frame_dots(frames, baseline)
        scales = torch.where(sums[N] == 0, torch.zeros_like(sums[:N]), sums[:N] / sums[N]).float()
    else:
        scales = torch.ones(N, dtype=torch.float32, device=frames.device)
    noise_k, ths = float(noise_k), float(ths)
    if noise_k != 0.0:
        m, lo = ops.temporal_select(frames, [quantile_rank(0.5, N), quantile_rank(0.1587, N)], a=scales, b=baseline)
        tau = (m + noise_k * (m - lo)) + ths
    else:
        tau = torch.full_like(baseline, ths) if ths != 0.0 else None
    sparse = ops.sparse_residual(frames, scales, baseline, tau, out=out, pair=pair)
    return SparseSplit(sparse, baseline, scales, tau)


Registration = namedtuple("Registration", ["frames", "shifts", "peak", "template"])


def taper_window(n, taper):
    """The raised-cosine edge taper of ``n`` samples as a float32 CPU tensor: 0.5 - 0.5 cos(pi (i + 0.5) / taper) on the first and
    (mirrored) the last ``taper`` samples, 1 between; formed in float64 and rounded once."""
    w = torch.ones(n, dtype=torch.float64)
    if taper:
        edge = 0.5 - 0.5 * torch.cos(math.pi * (torch.arange(taper, dtype=torch.float64) + 0.5) / taper)
        w[:taper] = edge
        w[n - taper:] = edge.flip(0)
    return w.to(torch.float32)


def _reg_args(stack, template, max_shift, taper, smooth, eps, chunk, what, item="frame", views=None):
    """The checks of the three estimators that need no device, for a stack of frames (``item`` "frame", or "view" with ``views`` =
    (centers, view_shape): window and taper are then a view's) or of volumes ("volume"): (max_shift and taper per axis, chunk,
    centers int32 [L,2] or None)."""
    rank = 3 if item == "volume" else 2
    layout, dtypes, word = ("[N,D,H,W]", (torch.float32,), "float32") if rank == 3 else ("[N,H,W]", (torch.float32, torch.float16), "float32 or float16")
    if not torch.is_tensor(stack) or stack.dim() != rank + 1 or not stack.is_contiguous():
        raise ValueError(f"{what}: a contiguous {layout} stack is expected")
    if stack.dtype not in dtypes:
        raise ValueError(f"{what}: a {word} stack is expected, got {stack.dtype}")
    sides = tuple(int(n) for n in stack.shape[1:])
    if template is not None and (not torch.is_tensor(template) or tuple(template.shape) != sides or template.dtype != torch.float32):
        raise ValueError(f"{what}: the template is a float32 {list(sides)} tensor, the shape of a {'volume' if rank == 3 else 'frame'}")
    c = None
    if views is not None:
        c, *sides = ops._view_centers(*views, what)
    m = ops._max_shift(max_shift, *sides, what)
    if rank == 2:                                                     # one width for both axes
        taper = (min(16, min(sides) // 8) if taper is None else int(taper),) * 2
        shown, size = taper[0], f"{sides[0]} x {sides[1]}"
    else:
        if taper is None:
            taper = tuple(min(16, n // 8) for n in sides)
        elif isinstance(taper, int):
            taper = (taper,) * 3
        else:
            taper = tuple(int(t) for t in taper)
            if len(taper) != 3:
                raise ValueError(f"{what}: taper is an int or (tz, ty, tx), got {taper!r}")
        shown, size = taper, tuple(sides)
    if any(t < 0 or 2 * t > n for t, n in zip(taper, sides)):
        raise ValueError(f"{what}: taper = {shown} does not fit a {size} {item} twice")
    smooth, eps = float(smooth), float(eps)
    if not 0.0 <= smooth < float("inf") or not 0.0 <= eps < float("inf"):
        raise ValueError(f"{what}: smooth and eps are finite and not negative, got {smooth}, {eps}")
    if chunk is None and views is not None:
        chunk = max(1, VIEW_CHUNK_BYTES // (len(c) * sides[0] * sides[1] * 4))
    if int(chunk) < 1:
        raise ValueError(f"{what}: chunk must be at least 1, got {chunk}")
    return m, taper, int(chunk), c


def _subpixel_arg(subpixel, upsample, what):
    """(dft, upsample): ``subpixel`` is True / False (the parabola through the integer peak, or nothing) or "dft"."""
    if isinstance(subpixel, str):
        if subpixel != "dft":
            raise ValueError(f"{what}: subpixel is True, False or 'dft', got {subpixel!r}")
        return True, ops._count(upsample, "upsample", what)
    return False, None


def _estimate(window, tapered, N, shape, max_shift, smooth, eps, subpixel, dft, upsample, chunk):
    """(shifts float32 [n, rank], peak float32 [n]), n = N x the items of a stack element: the phase correlation the three estimators
    share.  ``tapered``: the tapered float32 template, [*items, *shape] with ``shape`` the 2 or 3 transformed axes (items: nothing,
    L views, or the B blocks of a volume's grid); ``window(s, e, out)`` writes the tapered float32 elements s .. e - 1 of the stack into ``out`` [e - s, *items, *shape] and
    returns it.  The template is transformed, whitened and conjugated, low-passed where ``smooth`` > 0, its DC bin zeroed; a chunk
    is windowed, transformed, whitened against that plane, transformed back, and searched for its peak."""
    rank, dev = len(shape), tapered.device
    axes = tuple(range(-rank, 0))
    per = math.prod(tapered.shape[:-rank])
    T = torch.fft.rfftn(tapered, dim=axes).contiguous()
    U = torch.view_as_real(ops.reg_whiten(T, None, eps, out=T))
    if smooth > 0.0:
        k2 = None                                                     # the axes' squared frequencies, summed in axis order, float64
        for a, n in enumerate(shape):
            k = (torch.fft.rfftfreq if a == rank - 1 else torch.fft.fftfreq)(n, dtype=torch.float64)
            k = k.reshape([-1 if b == a else 1 for b in range(rank)]) ** 2
            k2 = k if k2 is None else k2 + k
        G = torch.exp(-2.0 * math.pi ** 2 * smooth ** 2 * k2).to(torch.float32).to(dev)
        Wt = torch.stack((U[..., 0] * G, -U[..., 1] * G), dim=-1)
    else:
        Wt = torch.stack((U[..., 0], -U[..., 1]), dim=-1)
    Wt[(..., *(0,) * rank, slice(None))] = 0.0                        # DC, per item
    Wt = torch.view_as_complex(Wt)
    shifts = torch.empty((N * per, rank), dtype=torch.float32, device=dev)
    ipeak = torch.empty((N * per, rank), dtype=torch.int32, device=dev)
    peak = torch.empty((N * per,), dtype=torch.float32, device=dev)
    chunk = min(chunk, max(N, 1))
    buf = torch.empty((chunk, *tapered.shape), dtype=torch.float32, device=dev)
    for s in range(0, N, chunk):
        e = min(s + chunk, N)
        a, b = s * per, e * per
        F = torch.fft.rfftn(window(s, e, buf[:e - s]), dim=axes).contiguous()  # (a no-op where rocFFT's layout is dense)
        corr = torch.fft.irfftn(ops.reg_whiten(F, Wt, eps, out=F), s=shape, dim=axes).reshape(b - a, *shape)
        (ops.reg_peak if rank == 2 else ops.reg_peak3d)(corr, max_shift, subpixel and not dft, out=(shifts[a:b], ipeak[a:b], peak[a:b]))
        if dft:                                                       # F is read again: irfft2 leaves its input alone (section 26.5)
            ops.reg_fine_peak(ops.reg_upsample(F.reshape(b - a, shape[0], shape[1] // 2 + 1), ipeak[a:b], shape, upsample), ipeak[a:b], upsample,
                              out=(shifts[a:b], peak[a:b]))
    return shifts, peak


@amp_region
def estimate_shifts(frames, template, max_shift=16, taper=None, smooth=0.0, eps=1e-5, subpixel=True, chunk=16, upsample=16):
    """(shifts float32 [N,2], peak float32 [N]) on the device: the rigid displacement (dy, dx) of every frame of a contiguous [N,H,W]
    fp32 / fp16 device stack against the float32 ``template`` [H,W] by phase correlation.  A frame that is
    the template displaced by d (frame[p] = template[p - d]) reports d; ``shift_frames`` undoes it.  ``peak`` is the correlation
    value at the integer peak (1 for a perfect cyclic copy).  Nothing is read back.

    Both get a raised-cosine edge taper of ``taper`` pixels (None: min(16, side / 8); 0: none); the spectra are whitened
    separately, F / (|F| + ``eps``), multiplied, optionally low-passed by a Gaussian of ``smooth`` pixels, and transformed back;
    the peak is searched over |dy| <= my, |dx| <= mx (``max_shift``: an int or (my, mx)) and, with ``subpixel``, refined by a
    parabola per axis.  ``subpixel="dft"``: the correlation is instead evaluated from the whitened spectra on a grid of
    1 / ``upsample`` px over +-1 px around the integer peak (an up-sampled DFT in float64, section 26.5) and the parabola is fitted
    on that grid; ``peak`` is then the fine maximum.  The frames go through in chunks of ``chunk`` (their spectra are
    chunk x H x (W/2+1) x 8 bytes)."""
    what = "estimate_shifts"
    m, (ty, tx), chunk, _ = _reg_args(frames, template, max_shift, taper, smooth, eps, chunk, what)
    dft, upsample = _subpixel_arg(subpixel, upsample, what)
    if template is None:
        raise ValueError(f"{what}: a template is needed")
    N, H, W = (int(s) for s in frames.shape)
    wy, wx = taper_window(H, ty).to(frames.device), taper_window(W, tx).to(frames.device)
    return _estimate(lambda s, e, out: ops.reg_window(frames[s:e], wy, wx, out=out), ops.reg_window(template.contiguous()[None], wy, wx)[0], N, (H, W),
                     m, smooth, eps, subpixel, dft, upsample, chunk)


@amp_region
def shift_frames(frames, shifts, mode="bilinear", fill=0.0, out=None):
    """out[n,y,x] = frames[n, y + dy, x + dx] with (dy, dx) = shifts[n] (float32 [N,2] on the device, as ``estimate_shifts`` returns
    them): bilinear, or ``mode="nearest"``; pixels from outside the frame are ``fill``.  An integer shift copies bits.  The result
    has the dtype of ``frames``; ``out`` must not share memory with ``frames``."""
    if not torch.is_tensor(frames) or frames.dim() != 3 or not frames.is_contiguous():
        raise ValueError("shift_frames: a contiguous [N,H,W] stack is expected")
    ops._shift_mode(mode, "shift_frames", plain=True)
    if not torch.is_tensor(shifts) or tuple(shifts.shape) != (int(frames.shape[0]), 2) or shifts.dtype != torch.float32:
        raise ValueError(f"shift_frames: shifts is a float32 [{int(frames.shape[0])}, 2] tensor")
    if out is not None and (out is frames or (torch.is_tensor(out) and ops._overlap(out, frames))):
        raise ValueError("shift_frames: out must not alias frames")
    return ops.reg_shift(frames, shifts, mode=mode, fill=fill, out=out)


def _register_args(stack, n_iter, mode, out, what, item="frame"):
    """The checks the three ``register_*`` add to their estimator's."""
    if int(n_iter) < 1:
        raise ValueError(f"{what}: n_iter must be at least 1, got {n_iter}")
    ops._shift_mode(mode, what, plain=True)
    if out is not None and (out is stack or (torch.is_tensor(out) and ops._overlap(out, stack))):
        raise ValueError(f"{what}: out must not alias {item}s")
    if int(stack.shape[0]) < 1:
        raise ValueError(f"{what}: at least one {item} is expected")


def _register(stack, template, n_iter, median, estimate, move, out):
    """(moved stack, the last estimate, the last template): ``estimate(template)`` measures the stack against a template --
    ``median(stack)`` where none is given -- and ``move(estimate, out)`` resamples THE ORIGINAL stack under it; with ``n_iter`` > 1
    the template becomes the median of the moved stack and both are done again, so interpolation never compounds."""
    tmpl = median(stack) if template is None else template
    for it in range(int(n_iter)):
        est = estimate(tmpl)
        out = move(est, out)
        if it + 1 < int(n_iter):
            tmpl = median(out)
    return out, est, tmpl


def _frame_median(frames):
    """The per-pixel lower temporal median of a [N,H,W] stack."""
    return ops.temporal_select(frames, [quantile_rank(0.5, int(frames.shape[0]))])[0]


@amp_region
def register_frames(frames, template=None, n_iter=1, max_shift=16, subpixel=True, mode="bilinear", taper=None, smooth=0.0, eps=1e-5,
                    chunk=16, fill=0.0, out=None, upsample=16):
    """Rigid registration of a contiguous [N,H,W] fp32 / fp16 device stack:
    ``Registration(frames, shifts, peak, template)`` with frames[n] = the input's frame n moved back by shifts[n].  ``template``
    None: the per-pixel temporal median of the stack.  ``n_iter`` > 1: the template becomes the median of the registered stack and
    the shifts are estimated again FROM THE ORIGINAL FRAMES, so interpolation never compounds.  The other arguments are those of
    ``estimate_shifts`` and ``shift_frames``.  Nothing is read back."""
    _reg_args(frames, template, max_shift, taper, smooth, eps, chunk, "register_frames")
    _subpixel_arg(subpixel, upsample, "register_frames")
    _register_args(frames, n_iter, mode, out, "register_frames")
    estimate = lambda tmpl: estimate_shifts(frames, tmpl, max_shift=max_shift, taper=taper, smooth=smooth, eps=eps, subpixel=subpixel, chunk=chunk,
                                            upsample=upsample)
    out, (shifts, peak), tmpl = _register(frames, template, n_iter, _frame_median, estimate,
                                          lambda est, out: shift_frames(frames, est[0], mode=mode, fill=fill, out=out), out)
    return Registration(out, shifts, peak, tmpl)


def valid_window(shifts, shape):
    """(y0, y1, x0, x1): the box of a frame of ``shape`` (H, W) in which every frame registered with ``shifts`` [N,2] holds data
    and no ``fill`` -- rows y0 .. y1 - 1, columns x0 .. x1 - 1 -- empty (all 0) where a shift is not finite or nothing is left.  A
    host helper: it reads the shifts back."""
    H, W = int(shape[0]), int(shape[1])
    s = torch.as_tensor(shifts).detach().to("cpu", torch.float64).reshape(-1, 2)
    if s.numel() == 0:
        return 0, H, 0, W
    if not bool(torch.isfinite(s).all()):
        return 0, 0, 0, 0
    lo, hi = torch.floor(s).amin(0), torch.ceil(s).amax(0)
    y0, y1 = max(0, int(-lo[0])), min(H, H - int(hi[0]))
    x0, x1 = max(0, int(-lo[1])), min(W, W - int(hi[1]))
    if y1 <= y0 or x1 <= x0:
        return 0, 0, 0, 0
    return y0, y1, x0, x1


# ------------------------------------------------------------------------------------------------ per-lenslet registration
ViewFit = namedtuple("ViewFit", ["table", "params", "inlier"])
ViewRegistration = namedtuple("ViewRegistration", ["frames", "table", "params", "shifts", "peak", "inlier", "template"])
VIEW_CHUNK_BYTES = 256 << 20          # the default chunk keeps the tapered views of a chunk at or below this


def view_labels(shape, centers, view_shape, device="cuda"):
    """uint8 [H,W] on the device: which lenslet view a pixel of a frame of ``shape`` belongs to.  View i is
    the box of ``view_shape`` (ph, pw) whose first row is centers[i][0] - ph // 2 (columns alike): for even sizes the box of
    ``extract_views``, for odd sizes not -- ``extract_views`` returns 2 (s // 2) pixels.  Where boxes overlap the pixel goes to the
    nearest centre (integer squared distance, ties to the lowest index); a pixel in no box gets L, the rest of the frame.  Computed
    once per geometry."""
    return ops.reg_label_map(shape, centers, view_shape, device)


@amp_region
def estimate_view_shifts(frames, template, centers, view_shape, max_shift=8, taper=None, smooth=0.0, eps=1e-5, subpixel=True, chunk=None,
                         upsample=16):
    """(shifts float32 [N,L,2], peak float32 [N,L]) on the device: ``estimate_shifts`` for every lenslet view of every frame against
    the same view of the float32 ``template`` [H,W].  ``centers``: an integer [L,2] host table of (row,
    column); ``view_shape`` (ph, pw): the boxes of ``view_labels``, read as 0 outside the frame.  The views are cut, widened and
    tapered in one read of the stack (``taper`` None: min(16, side / 8) of a view); whitening, the peak (|dy| <= my, |dx| <= mx of
    ``max_shift``), the parabola and the up-sampled DFT are the kernels of ``estimate_shifts`` on the batch of views.  ``chunk`` is in
    FRAMES: a chunk holds chunk x L x ph x pw x 4 bytes of tapered views plus their spectra, chunk x L x ph x (pw/2+1) x 8 bytes, and
    the correlation maps; None keeps the views at or below 256 MiB.  Nothing is read back."""
    what = "estimate_view_shifts"
    m, (ty, tx), chunk, c = _reg_args(frames, template, max_shift, taper, smooth, eps, chunk, what, "view", (centers, view_shape))
    dft, upsample = _subpixel_arg(subpixel, upsample, what)
    if template is None:
        raise ValueError(f"{what}: a template is needed")
    N, L, (ph, pw) = int(frames.shape[0]), len(c), (int(v) for v in view_shape)
    wy, wx = taper_window(ph, ty).to(frames.device), taper_window(pw, tx).to(frames.device)
    shifts, peak = _estimate(lambda s, e, out: ops.reg_window_views(frames[s:e], c, (ph, pw), wy, wx, out=out),
                             ops.reg_window_views(template.contiguous()[None], c, (ph, pw), wy, wx)[0], N, (ph, pw), m, smooth, eps, subpixel, dft,
                             upsample, chunk)
    return shifts.reshape(N, L, 2), peak.reshape(N, L)


def _directions(directions, c, device, what):
    """float64 [L,2] on the device: the given directions, or centers - mean(centers)."""
    if directions is None:
        g = torch.from_numpy(c).to(torch.float64)
        return (g - g.mean(dim=0, keepdim=True)).to(device)
    g = torch.as_tensor(directions)
    if tuple(g.shape) != (len(c), 2) or not (g.is_floating_point() or g.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"{what}: directions is a [{len(c)}, 2] table, one (row, column) vector per view")
    return g.to(device=device, dtype=torch.float64).contiguous()


def fit_view_shifts(shifts, peak, directions, min_peak=0.0, reject=1.0, model="axial"):
    """``ViewFit(table, params, inlier)`` from the per-view shifts of ``estimate_view_shifts``: per frame the lateral displacement d
    and the axial coefficient a of s_i = d + a g_i (``directions`` g: [L,2], converted to float64), fitted in float64 over the views
    whose peak is finite and >= ``min_peak``, with one rejection pass at ``reject`` pixels.  ``params``
    float64 [N,3] = (d_y, d_x, a) -- a is a z-drift monitor in its own right; ``inlier`` uint8 [N,L]; ``table`` float32 [N,L+1,2]:
    the shift of every view (``model="axial"``: the model's; ``"free"``: the measured one where it is an inlier) and, in row L, of
    the rest of the frame (d).  Everything stays on the device."""
    if not torch.is_tensor(shifts) or not shifts.is_cuda:
        raise RuntimeError("fit_view_shifts: cwfa_amd runs on MI355X only -- shifts must be a device tensor (no CPU fallback exists)")
    if shifts.dim() != 3:
        raise ValueError("fit_view_shifts: shifts is a float32 [N,L,2] tensor")
    g = torch.as_tensor(directions)
    if tuple(g.shape) != (int(shifts.shape[1]), 2):
        raise ValueError(f"fit_view_shifts: directions is a [{int(shifts.shape[1])}, 2] table, one (row, column) vector per view")
    g = g.to(device=shifts.device, dtype=torch.float64).contiguous()
    return ViewFit(*ops.reg_fit_views(shifts, peak, g, min_peak, reject, model))


@amp_region
def shift_views(frames, table, labels, mode="bilinear", fill=0.0, out=None):
    """out[n,y,x] = frames[n, y + dy, x + dx] with (dy, dx) = table[n, min(labels[y,x], L)]: ``shift_frames`` with a shift per lenslet
    view (``table`` float32 [N,L+1,2] of ``fit_view_shifts``, ``labels`` uint8 [H,W] of ``view_labels``).  The source is the whole
    frame: a tap that leaves its view's box reads what lies there (``valid_view_windows`` gives the part of every view where none
    does).  An integer shift copies bits; ``out`` must not share memory with ``frames``."""
    if not torch.is_tensor(frames) or frames.dim() != 3 or not frames.is_contiguous():
        raise ValueError("shift_views: a contiguous [N,H,W] stack is expected")
    ops._shift_mode(mode, "shift_views", plain=True)
    N, H, W = (int(s) for s in frames.shape)
    if not torch.is_tensor(table) or table.dim() != 3 or int(table.shape[0]) != N or table.shape[2] != 2 or table.dtype != torch.float32:
        raise ValueError(f"shift_views: table is a float32 [{N}, L + 1, 2] tensor")
    if not torch.is_tensor(labels) or tuple(labels.shape) != (H, W) or labels.dtype != torch.uint8:
        raise ValueError(f"shift_views: labels is a uint8 [{H}, {W}] map")
    if out is not None and (out is frames or (torch.is_tensor(out) and ops._overlap(out, frames))):
        raise ValueError("shift_views: out must not alias frames")
    return ops.reg_shift_labeled(frames, table, labels, mode=mode, fill=fill, out=out)


@amp_region
def register_views(frames, centers, view_shape, template=None, directions=None, model="axial", n_iter=1, max_shift=8, subpixel=True,
                   mode="bilinear", taper=None, smooth=0.0, eps=1e-5, chunk=None, fill=0.0, out=None, upsample=16, min_peak=0.0, reject=1.0,
                   labels=None):
    """Per-lenslet registration of a contiguous [N,H,W] fp32 / fp16 device stack:
    ``ViewRegistration(frames, table, params, shifts, peak, inlier, template)``.  Every view of every frame is registered against the
    same view of the template, the L shifts of a frame are fitted by a lateral displacement plus an axial fan a g_i
    (``directions`` g; None: centers - mean(centers)), and every pixel is moved back by its view's vector (the rest of the frame by
    d).  ``template`` None: the per-pixel temporal median; ``n_iter`` > 1: the template becomes the median of the registered stack
    and the shifts are estimated again FROM THE ORIGINAL FRAMES.  ``labels``: the map of ``view_labels`` where it is at hand.  The
    other arguments are those of ``estimate_view_shifts``, ``fit_view_shifts`` and ``shift_views``.  Nothing is read back."""
    what = "register_views"
    c = _reg_args(frames, template, max_shift, taper, smooth, eps, chunk, what, "view", (centers, view_shape))[3]
    _subpixel_arg(subpixel, upsample, what)
    _register_args(frames, n_iter, mode, out, what)
    if model not in ("axial", "free"):
        raise ValueError(f"{what}: model is 'axial' or 'free', got {model!r}")
    g = _directions(directions, c, frames.device, what)
    if labels is None:
        labels = view_labels(frames.shape[1:], c, view_shape, frames.device)

    def estimate(tmpl):
        shifts, peak = estimate_view_shifts(frames, tmpl, c, view_shape, max_shift=max_shift, taper=taper, smooth=smooth, eps=eps, subpixel=subpixel,
                                            chunk=chunk, upsample=upsample)
        return shifts, peak, fit_view_shifts(shifts, peak, g, min_peak=min_peak, reject=reject, model=model)

    out, (shifts, peak, fit), tmpl = _register(frames, template, n_iter, _frame_median, estimate,
                                               lambda est, out: shift_views(frames, est[2].table, labels, mode=mode, fill=fill, out=out), out)
    return ViewRegistration(out, fit.table, fit.params, shifts, peak, fit.inlier, tmpl)


def valid_view_windows(table, centers, view_shape, shape):
    """int [L,4] rows (y0, y1, x0, x1) in FRAME coordinates: per view, the box in which every frame's taps under ``table`` [N,L+1,2]
    stay inside that view's box and inside the frame -- rows y0 .. y1 - 1, columns x0 .. x1 - 1; all 0 where a shift of the view is
    not finite or nothing is left.  (Where boxes overlap, a pixel of that window may carry another view's label.)  A host helper: it
    reads the table back, like ``valid_window``."""
    import numpy as np
    c, ph, pw = ops._view_centers(centers, view_shape, "valid_view_windows")
    H, W = int(shape[0]), int(shape[1])
    t = torch.as_tensor(table).detach().to("cpu", torch.float64)
    if t.dim() != 3 or t.shape[1] != len(c) + 1 or t.shape[2] != 2:
        raise ValueError(f"valid_view_windows: table is a [N, {len(c) + 1}, 2] tensor")
    t = t.numpy()
    out = np.zeros((len(c), 4), dtype=np.int64)
    for i in range(len(c)):
        by0, bx0 = int(c[i, 0]) - ph // 2, int(c[i, 1]) - pw // 2
        lo, hi = (max(by0, 0), max(bx0, 0)), (min(by0 + ph, H), min(bx0 + pw, W))
        s = t[:, i]
        if s.size:
            if not np.isfinite(s).all():
                continue
            fl, ce = np.floor(s).min(0), np.ceil(s).max(0)
            lo = (max(lo[0], lo[0] - int(fl[0])), max(lo[1], lo[1] - int(fl[1])))
            hi = (min(hi[0], hi[0] - int(ce[0])), min(hi[1], hi[1] - int(ce[1])))
        if hi[0] > lo[0] and hi[1] > lo[1]:
            out[i] = lo[0], hi[0], lo[1], hi[1]
    return out


def _scalar(v):
    """A float64 statistic as the 0-dim float32 CPU tensor the reference returns (rounded once)."""
    return torch.tensor(v, dtype=torch.float64).to(torch.float32)


def _channels(ds):
    """The image tensors behind the two statistics channels of a dataset: (views, views) for [N,H,W], the strided copies of
    [..., 0] and [..., 1] for the sparse [N,H,W,2] layout."""
    sv = ds.stacked_views
    if sv.dim() == 4:
        return sv[..., 0].contiguous(), sv[..., 1].contiguous()
    return sv, sv


def _max(t):
    return ops.volume_extrema(t.reshape(1, 1, 1, -1) if t.is_contiguous() else t.contiguous().reshape(1, 1, 1, -1))[0, 1].cpu()


def shot_noise_scales(m, u, signal_power_range):
    """(pre, post) of the shot-noise augmentation for image maxima ``m`` and uniforms ``u`` (two tensors of one shape, any device):
    the signal power P = lo + (hi - lo) u photons at the image's maximum, pre = P / m and post = m / P, both 0 where m <= 0 (an
    all-zero image stays all zero instead of becoming NaN).  Plain torch, fp32."""
    lo, hi = (float(v) for v in signal_power_range)
    if not 0.0 < lo <= hi or hi == float("inf"):
        raise ValueError(f"add_random_shot_noise_to_dataset: signal_power_range {list(signal_power_range)} is not 0 < lo <= hi < inf")
    P = lo + (hi - lo) * u
    lit = m > 0
    safe = torch.where(lit, m, torch.ones_like(m))
    zero = torch.zeros_like(m)
    return torch.where(lit, P / safe, zero), torch.where(lit, safe / P, zero)


class XLFMDatasetFull:
    """The tensor side of the reference's dataset class: ``stacked_views`` (fp32 [N,H,W]) and ``vols`` on the HIP device."""
    extract_views = staticmethod(extract_views)

    def __init__(self, stacked_views=None, vols=None, ds_id=""):
        self.stacked_views, self.vols, self.dataset_id = stacked_views, vols, ds_id
        self.load_vols = vols is not None
        self.gt_cache = []

    @classmethod
    def from_tensors(cls, raw_frames, vols, img_shape, ds_id="", sparse=None):
        """From raw fp32 frames [N,h,w] and fp16 volumes [N,D,H0,W0] as read from the files.  ``sparse``: True, or a dict of
        ``extract_sparse`` arguments: ``stacked_views`` is then the sparse component of the prepared frames ([N,H,W], or the
        [N,H,W,2] pair with ``pair=True``) -- what the reference reads from ``SLNet_preprocessed/``."""
        frames = prepare_frames(raw_frames, img_shape)
        if sparse is None or sparse is False:
            return cls(frames, vols, ds_id)
        kw = {} if sparse is True else dict(sparse)
        if "out" not in kw and not kw.get("pair", False):
            kw["out"] = frames                                      # the prepared frames are ours: in place
        return cls(extract_sparse(frames, **kw).sparse, vols, ds_id)

    @classmethod
    def from_tensors_registered(cls, raw_frames, vols, img_shape, ds_id="", register=True, sparse=None):
        """``from_tensors`` with rigid registration of the prepared frames BEFORE ``sparse``: ``register`` is True or a dict of
        ``register_frames`` arguments (None / False: exactly ``from_tensors``).  The dataset carries the ``Registration`` (without
        its frames) as ``registration``.  (``from_tensors`` keeps its signature: this is its registering form.)"""
        if register is None or register is False:
            return cls.from_tensors(raw_frames, vols, img_shape, ds_id, sparse)
        reg = register_frames(prepare_frames(raw_frames, img_shape), **({} if register is True else dict(register)))
        frames = reg.frames
        if sparse is not None and sparse is not False:
            kw = {} if sparse is True else dict(sparse)
            if "out" not in kw and not kw.get("pair", False) and frames.dtype == torch.float32:
                kw["out"] = frames                                  # the registered frames are ours: in place
            frames = extract_sparse(frames, **kw).sparse
        ds = cls(frames, vols, ds_id)
        ds.registration = reg._replace(frames=None)
        return ds

    def __len__(self):
        return int(self.stacked_views.shape[0])

    def __getitem__(self, index):
        views_out = self.stacked_views[[index], ...]
        if not self.load_vols:
            return views_out
        return views_out, self.vols[index, ...], index, self.gt_cache

    def get_n_depths(self):
        return self.vols.shape[1]

    def get_max(self):
        m = _max(self.stacked_views.float())
        return m, m, _max(self.vols.float())

    def get_statistics(self):
        mi, si, _ = ops.mean_std([self.stacked_views.float()])
        mv, sv, _ = ops.mean_std([self.vols.float()])
        return _scalar(mi), _scalar(si), _scalar(mv), _scalar(sv)

    def standarize(self, stats):
        mean_imgs, std_imgs, mean_imgs_s, std_imgs_s, mean_vols, std_vols = stats
        self.stacked_views = self.standarize_sample(self.stacked_views, mean_imgs, std_imgs)
        self.vols = self.standarize_sample(self.vols, mean_vols, std_vols)

    @amp_function
    def add_random_shot_noise_to_dataset(self, signal_power_range=[32**2, 32**2], seed=None, sample_offset=0):
        """Photon shot noise on every image of ``stacked_views`` ([N,H,W]), in place, on the device, nothing read back: image i is
        scaled so that its maximum m_i holds P_i photons, P_i uniform in ``signal_power_range`` (photons at the brightest pixel; the
        default 32^2 gives a peak signal-to-noise ratio of 32), every pixel is replaced by a Poisson draw at that rate, and the
        image is scaled back:  views[i] <- Poisson(views[i] * P_i / m_i) * m_i / P_i.  An all-zero image stays all zero.
        Meant for NON-NEGATIVE images, i.e. before ``standarize``: a negative pixel becomes NaN.
        ``seed``: the draw is a pure function of (seed, sample_offset + i, pixel): u_i is ``ops.rand_uniform`` on stream 1, the
        Poisson draw ``ops.rand_poisson`` on stream 0.  None takes a seed from torch's generator, so ``set_all_seeds`` governs it.
        ``sample_offset``: the number of images in front of this dataset (``add_random_shot_noise_to_datasets`` passes it), so that the noise of an
        image does not depend on how the datasets were split."""
        v = self.stacked_views
        if v.dim() != 3:
            raise ValueError(f"add_random_shot_noise_to_dataset: expected stacked_views [N,H,W], got {tuple(v.shape)}")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())          # torch's CPU generator: no device read-back
        if v.dtype != torch.float32 or not v.is_contiguous():
            v = self.stacked_views = v.float().contiguous()
        N = int(v.shape[0])
        if v.numel() == 0:
            return
        m = ops.volume_extrema(v.reshape(N, 1, 1, -1))[:, 1]
        u = ops.rand_uniform((N, 1), seed, stream=1, sample_offset=sample_offset, device=v.device)[:, 0]
        pre, post = shot_noise_scales(m, u, signal_power_range)
        ops.rand_poisson(v, seed, stream=0, sample_offset=sample_offset, pre=pre.contiguous(), post=post.contiguous(), out=v)

    @staticmethod
    def standarize_sample(sample, mean, std):
        """(sample - mean) / std in fp32, in place where ``sample`` is contiguous."""
        return ops.prep_apply(sample if sample.is_contiguous() else sample.contiguous(), "sub_div", mean, std)

    @staticmethod
    def extract_views_normalized(image, lenslet_coords, subimage_shape, mean_imgs, std_imgs):
        """extract_views followed by ``(views - mean_imgs) / std_imgs`` (CWFA.py:796-797), fused."""
        return ops.extract_views(image, lenslet_coords, subimage_shape, float(mean_imgs), float(std_imgs))


class ConcatDataset:
    """XLFMDataset.py:251-395 over datasets whose ``stacked_views`` and ``vols`` are fp32 tensors on the HIP device.  The statistics
    are float64 device sums accumulated over the datasets (nothing is concatenated) and come back as 0-dim float32 CPU tensors,
    rounded once.  ``add_random_shot_noise_to_dataset`` (:397-405) calls a dataset method the reference does not define, so the class
    does not carry it; the augmentation it documents is the module's ``add_random_shot_noise_to_datasets(concat, ...)`` over
    ``XLFMDatasetFull.add_random_shot_noise_to_dataset``."""

    def __init__(self, *datasets):
        self.datasets = datasets
        self.max_values = None

    def _locate(self, i):
        for n, d in enumerate(self.datasets):
            if i < len(d) or n == len(self.datasets) - 1:
                return n, i
            i -= len(d)

    def __getitem__(self, input):
        n, i = self._locate(input)
        return tuple(self.datasets[n][i])

    def __len__(self):
        return sum(len(d) for d in self.datasets)

    @amp_function
    def mean_std(self, dim=0):
        """``(mean(dim), std(dim))`` from ONE pass over the volumes: the kernel produces both, and ``mean`` / ``std`` each take
        their half of it, so a caller that wants both asks here.  Several datasets are concatenated for the pass (the kernel
        reads one stack); a single dataset is read in place."""
        if dim != 0:
            raise NotImplementedError("ConcatDataset.mean / std: over the samples (dim=0) only")
        vols = [d.vols.float() for d in self.datasets]
        m, s = ops.stack_mean_std(vols[0] if len(vols) == 1 else torch.cat(vols, dim=0))
        return m.unsqueeze(0), s.unsqueeze(0)

    def mean(self, dim=0):
        """The per-voxel mean over all samples, [1,D,H,W] like the reference's permuted result."""
        return self.mean_std(dim)[0]

    def std(self, dim=0):
        return self.mean_std(dim)[1]

    @amp_function
    def get_statistics(self):
        """mean_imgs, std_imgs, mean_imgs_s, std_imgs_s, mean_vols, std_vols (unbiased std over every element of every dataset)."""
        chans = [_channels(d) for d in self.datasets]
        mi, si, _ = ops.mean_std([c[0] for c in chans])
        if self.datasets[0].stacked_views.dim() == 4:
            ms, ss, _ = ops.mean_std([c[1] for c in chans])
        else:
            ms, ss = mi, si
        mv, sv, _ = ops.mean_std([d.vols.float() for d in self.datasets])
        return _scalar(mi), _scalar(si), _scalar(ms), _scalar(ss), _scalar(mv), _scalar(sv)

    @amp_function
    def get_max(self):
        if self.max_values is None:
            chans = [_channels(d) for d in self.datasets]
            self.max_values = [torch.stack([_max(c[0]) for c in chans]).max()]
            # the dense layout has one image channel: its maximum serves both entries, one extrema pass per dataset
            sparse = self.datasets[0].stacked_views.dim() == 4
            self.max_values.append(torch.stack([_max(c[1]) for c in chans]).max() if sparse else self.max_values[0].clone())
            self.max_values.append(torch.stack([_max(d.vols.float()) for d in self.datasets]).max())
        return self.max_values

    @amp_function
    def normalize_datasets(self):
        """Every dataset scaled to the common maxima: x / max(x) * max_values in fp32, in place.  In the sparse layout channel 0 takes
        ``max_values[1]`` and channel 1 ``max_values[0]``, as in the reference."""
        if self.max_values is None:
            self.max_values = self.get_max()
        for d in self.datasets:
            if d.stacked_views.dim() == 4:
                for k in (0, 1):
                    c = d.stacked_views[..., k].contiguous()
                    d.stacked_views[..., k] = ops.prep_apply(c, "div_mul", _max(c), self.max_values[1 - k])
            else:
                v = d.stacked_views.float()
                d.stacked_views = ops.prep_apply(v if v.is_contiguous() else v.contiguous(), "div_mul", _max(v), self.max_values[0])
            v = d.vols.float()
            v = v if v.is_contiguous() else v.contiguous()
            d.vols = ops.prep_apply(v, "div_mul", _max(v), self.max_values[2])

    @amp_function
    def standarize_datasets(self, stats=None):
        if stats is None:
            stats = self.get_statistics()
        for d in self.datasets:
            d.standarize(stats)


def add_random_shot_noise_to_datasets(datasets, signal_power_range=[32**2, 32**2], seed=None):
    """What the reference's ``ConcatDataset.add_random_shot_noise_to_dataset`` (:397-405) is documented to do, as a function of a
    ``ConcatDataset`` or a sequence of ``XLFMDatasetFull``: shot noise on every dataset under ONE seed (None: from torch's
    generator), each with ``sample_offset`` set to the number of images in front of it, so that the result is that of the unsplit
    stack, bit for bit."""
    if seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
    offset = 0
    for d in getattr(datasets, "datasets", datasets):
        d.add_random_shot_noise_to_dataset(signal_power_range=signal_power_range, seed=seed, sample_offset=offset)
        offset += len(d)
