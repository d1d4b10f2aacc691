"""Plain numpy / torch restatement of the data preparation pass, the yardstick of tests/test_prep_cpu.py and
tests/test_gpu_prep.py: the crop offsets, the threshold modes on fp16 values, the frame clean-up and index map, torch.histogram's
CPU bin rule, the quantile walk, and float64 two-pass moments.  Nothing here calls the package under test."""
import numpy as np
import torch


# ---------------------------------------------------------------------------------------------- index maps
def crop_range(full, crop):
    c = full // 2
    return c - crop // 2, c + -(-crop // 2)


def frame_offsets(h, w, S0, S1):
    """(oy, ox): output (r, c) of pad-to-min + centre crop is source (r + oy, c + ox).  The pad is the floor-halved negative
    difference to the shorter side, taken off both sides."""
    m = min(h, w)
    ph, pw = -((m - h) // 2), -((m - w) // 2)
    h1, w1 = h - 2 * ph, w - 2 * pw
    return ph + (h1 - S0) // 2, pw + (w1 - S1) // 2


# ---------------------------------------------------------------------------------------------- volumes
def f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def prep_volumes(vol16, H, W, volume_ths, norm):
    """vol16: float16 [N,D,H0,W0] -> float16 [N,D,H,W]; every comparison in fp32, every stored value rounded to fp16."""
    (h0, h1), (w0, w1) = crop_range(vol16.shape[2], H), crop_range(vol16.shape[3], W)
    v = vol16[:, :, h0:h1, w0:w1].copy()
    f = v.astype(np.float32)
    if norm == "max":
        q = (f / f.max()).astype(np.float16)                      # fp32 quotient, one rounding to fp16
        q[q.astype(np.float32) < np.float32(np.float16(volume_ths))] = 0
        return q
    if norm is not None:
        raise NotImplementedError(norm)
    if isinstance(volume_ths, float):
        thr = np.float32(volume_ths) * f.max()                    # fp32 product
        v[f <= thr] = 0
    elif len(volume_ths) == 2:
        v[f < np.float32(volume_ths[0])] = 0
        v[v.astype(np.float32) >= np.float32(volume_ths[1])] = np.float16(volume_ths[1])
    return v


# ---------------------------------------------------------------------------------------------- frames
def prep_frames(raw, S0, S1):
    raw = np.asarray(raw, dtype=np.float32)
    N, h, w = raw.shape
    x = np.where(np.isnan(raw), np.float32(0), raw)
    x = np.minimum(np.maximum(x, np.float32(0)), np.float32(50000))
    x = x.astype(np.float16).astype(np.float32)
    oy, ox = frame_offsets(h, w, S0, S1)
    out = np.zeros((N, S0, S1), np.float32)
    r, c = np.arange(S0) + oy, np.arange(S1) + ox
    rv, cv = (r >= 0) & (r < h), (c >= 0) & (c < w)
    out[np.ix_(np.arange(N), np.nonzero(rv)[0], np.nonzero(cv)[0])] = x[np.ix_(np.arange(N), r[rv], c[cv])]
    return out


# ---------------------------------------------------------------------------------------------- histogram
def hist_range(lo, hi):
    lo, hi = np.float32(lo), np.float32(hi)
    if lo == hi:
        lo, hi = np.float32(lo - np.float32(0.5)), np.float32(hi + np.float32(0.5))
    return lo, hi


def hist_edges(lo, hi, bins):
    return torch.linspace(torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32), bins + 1, dtype=torch.float32).numpy()


def hist_bins(x, lo, hi, edges):
    """The bin of every element (all inside [lo, hi]): position by separately rounded fp32 operations, then the last edge <= x
    among edges[pos-1 .. pos+1]; the top edge belongs to the last bin."""
    x = np.asarray(x, dtype=np.float32).ravel()
    bins = len(edges) - 1
    lo, hi = np.float32(lo), np.float32(hi)
    pos = ((x - lo) / np.float32(hi - lo) * np.float32(bins)).astype(np.int64)
    pos = np.clip(pos, 0, bins)
    a, b = np.maximum(pos - 1, 0), np.minimum(pos + 2, bins + 1)
    cnt = np.zeros_like(pos)
    for k in range(3):
        idx = a + k
        cnt += (idx < b) & (edges[np.minimum(idx, bins)] <= x)
    return np.clip(a + cnt - 1, 0, bins - 1)


def hist_bins_plain(x, lo, hi, bins):
    """The position alone, WITHOUT the search among the edges: what must not ship (wrong near every edge)."""
    x = np.asarray(x, dtype=np.float32).ravel()
    pos = ((x - np.float32(lo)) / np.float32(np.float32(hi) - np.float32(lo)) * np.float32(bins)).astype(np.int64)
    return np.clip(pos, 0, bins - 1)


def histogram(x, bins, lo=None, hi=None):
    """(int64 counts, float32 edges) as torch.histogram(x, bins) gives on the CPU."""
    x = np.asarray(x, dtype=np.float32).ravel()
    lo, hi = hist_range(x.min() if lo is None else lo, x.max() if hi is None else hi)
    edges = hist_edges(lo, hi, bins)
    keep = (x >= lo) & (x <= hi)
    return np.bincount(hist_bins(x[keep], lo, hi, edges), minlength=bins).astype(np.int64), edges


# ---------------------------------------------------------------------------------------------- quantile walk
def quantile_walk(counts, edges, quant):
    """The walk over bins 1 .. bins-1 in fp32: stop before adding bin n once the bins before it hold sum(counts[1:]) * quant; the
    result is that bin's lower edge.  Returns (edge, n_bin, crossed, margin_above, margin_below)."""
    h = torch.as_tensor(np.asarray(counts)).to(torch.float32)
    target = h[1:].sum() * quant
    cum, prev, crossed = torch.zeros((), dtype=torch.float32), torch.zeros((), dtype=torch.float32), False
    n_bin = 0
    for n_bin in range(1, len(h)):
        if cum >= target:
            crossed = True
            break
        prev = cum
        cum = cum + h[n_bin]
    return np.float32(edges[n_bin]), n_bin, crossed, float(cum - target), float(target - prev)


# ---------------------------------------------------------------------------------------------- moments
def mean_std(arrays):
    """Float64 two-pass mean and unbiased std over every element of the given arrays."""
    n = sum(a.size for a in arrays)
    mean = sum(np.asarray(a, np.float64).sum() for a in arrays) / n
    ss = sum(((np.asarray(a, np.float64) - mean) ** 2).sum() for a in arrays)
    return mean, (np.sqrt(ss / (n - 1)) if n > 1 else np.nan), n


def stack_mean_std(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x.mean(0), (x.std(0, ddof=1) if x.shape[0] > 1 else np.full(x.shape[1:], np.nan))


def apply(x, mode, a=0.0, b=0.0, upper=True, lower=True):
    x = np.asarray(x, np.float32).copy()
    a, b = np.float32(a), np.float32(b)
    if mode == "sub_div":
        return (x - a) / b
    if mode == "div_mul":
        return x / a * b
    if upper:
        x[x > a] = a
    if lower:
        x[x < b] = 0
    return x


# ---------------------------------------------------------------------------------------------- the whole preparation
def prepare(vol16, views, size, volume_ths, volume_quantiles, img_ths, norm):
    """load_XLFM_data behind the dataset object: (vols fp32, views fp32, upper clamp or None, image threshold)."""
    vols = prep_volumes(vol16, size[0], size[1], volume_ths, norm).astype(np.float32)
    upper = None
    if volume_quantiles[1] != 1:
        counts, edges = histogram(vols, 10000)
        upper = quantile_walk(counts, edges, volume_quantiles[1])[0]
        vols = apply(vols, "clamp_zero", a=upper, lower=False)
    low = np.float32(np.float32(views.max()) * np.float32(img_ths[0]))
    return vols, apply(views, "clamp_zero", b=low, upper=False), upper, low
