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
           "extract_sparse", "SparseSplit", "quantile_rank"]


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
