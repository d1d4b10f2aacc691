"""CPU restatement of the evaluation pass, test infrastructure beside split_ref.py: what the reference's
compute_INN_step_performance (CWFA.py:98-132), psnr (utils.py:380-394), volume_2_projections (utils.py:281-327), corr_coeff_3D
(CWFA.py:240-379) and norm_data / filter_data (utils.py:419-446) compute, written from their definitions.  Element-wise steps
are done in fp32 exactly as there (they are compared bit for bit); every sum is float64 (compared to 1e-8)."""
import numpy as np

F = np.float32


def raw_volume(x, step, mean, std):
    """(x / 2**step) * std - mean in fp32, each operation rounded (CWFA.py:112-113)."""
    x = np.asarray(x, dtype=F)
    return (x / F(2 ** step)) * F(std) - F(mean)


def extrema(a, b=None):
    """Per sample [B, 12]: min, max, min|.|, max|.| of a; of b; min, max of |a - b|; 0, 0."""
    a = np.asarray(a, dtype=F)
    out = np.zeros((a.shape[0], 12), dtype=F)
    for s in range(a.shape[0]):
        row = [a[s].min(), a[s].max(), np.abs(a[s]).min(), np.abs(a[s]).max()]
        if b is not None:
            bb = np.asarray(b, dtype=F)[s]
            d = np.abs(a[s] - bb)
            row += [bb.min(), bb.max(), np.abs(bb).min(), np.abs(bb).max(), d.min(), d.max()]
        out[s, :len(row)] = row
    return out


def metric_sums(pred, gt, thr=-np.inf):
    """float64 [B, 4]: sum (g-p)^2, sum g, sum |g - p~| with p~ = (p < thr ? 0 : p), #{p < thr} (CWFA.py:126-128)."""
    p, g = np.asarray(pred, dtype=F), np.asarray(gt, dtype=F)
    out = np.zeros((p.shape[0], 4))
    for s in range(p.shape[0]):
        pd_, gd = p[s].astype(np.float64).ravel(), g[s].astype(np.float64).ravel()
        mask = p[s].ravel() < F(thr)
        out[s] = [np.sum((gd - pd_) ** 2), np.sum(gd), np.sum(np.abs(gd - np.where(mask, 0.0, pd_))), mask.sum()]
    return out


def psnr_from(sse, sum_img1, numel, pixel_max=1.0):
    if sse == 0:
        return 0.0 if sum_img1 == 0 else 100.0
    return 20.0 * np.log10(pixel_max / np.sqrt(sse / numel))


def step_performance(gt, pred, step, mean, std, normalize_before=False, ths=0.05):
    """(psnr, masked MAE * 100, gt_raw, pred_raw); ths == 0: no mask (the reference itself raises there)."""
    g, p = raw_volume(gt, step, mean, std), raw_volume(pred, step, mean, std)
    if normalize_before:
        g, p = g - g.min(), p - p.min()
    thr = -np.inf if ths == 0 else F(np.abs(p).max()) * F(ths)
    sums = metric_sums(p, g, thr).sum(0)
    return psnr_from(sums[0], sums[1], g.size), sums[2] / g.size * 100.0, g, p


def volume_maps(v, normalize=False, ths=(0.0, 1.0)):
    """|v| and then the maps of utils.py:293-303 in fp32, in their order."""
    v = np.abs(np.asarray(v, dtype=F))
    if normalize:
        v = v - v.min()
        v = v / v.max()
    if ths[0] != 0.0 or ths[1] != 1.0:
        vmin, vmax = v.min(), v.max()
        rng = F(vmax - vmin)
        v = v.copy()
        v[(v - vmin) < F(rng * F(ths[0]))] = 0
        v[(v - vmin) > F(rng * F(ths[1]))] = F(vmin + F(rng * F(ths[1])))
    return v


def mip3(v):
    """Maximum projections of a non-negative [B,D,H,W] array: over depth [B,H,W], over H [B,W,D], over W [B,H,D], min [B]."""
    return v.max(1), v.max(2).transpose(0, 2, 1), v.max(3).transpose(0, 2, 1), v.reshape(v.shape[0], -1).min(1)


def nearest(n_out, n_in):
    """ATen's nearest-neighbour source indices: identity, halving, or min(floor(dst * fp32(in / out)), in - 1)."""
    scale = F(n_in) / F(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F) * scale).astype(np.int64), n_in - 1)


def compose(zp, xp, yp, depth_scale=2, border=2, bars=False):
    """utils.py:305-325 for scaling_factors [1, 1, depth_scale] and a square plane: [B, 1, H + s + border, W + s + border]."""
    B, H, W = zp.shape
    D = xp.shape[2]
    s = D * depth_scale
    out = np.full((B, 1, H + s + border, W + s + border), zp.min(), dtype=F)
    idx = nearest(s, D)
    out[:, 0, :H, :W] = zp
    out[:, 0, H + border:, :W] = xp.transpose(0, 2, 1)[:, idx, :]
    out[:, 0, :H, W + border:] = yp[:, :, idx]
    if bars:
        out[:, :, H:H + border, :] = 1.0
        out[:, :, :, W:W + border] = 1.0
    return out


def projections(vol_bdhw, depth_scale=2, ths=(0.0, 1.0), normalize=False, border=2, bars=False):
    """volume_2_projections of a depth-major [B,D,H,W] volume."""
    return compose(*mip3(volume_maps(vol_bdhw, normalize, ths))[:3], depth_scale, border, bars)


def roi_boxes(coords, shape, r12, r3, start_plane_offset=-25 // 2):
    _, D, H, W = shape
    out = np.zeros((len(coords), 6), dtype=np.int32)
    for i, (x, y, z) in enumerate(coords):
        z = z + D // 2 + start_plane_offset
        for k, (c, r, n) in enumerate(((z, r3, D), (y, r12, H), (x, r12, W))):
            lo, hi = max(0, int(c) - r), min(n, int(c) + r)
            if hi > lo:
                out[i, 2 * k:2 * k + 2] = lo, hi
    return out


def roi_means(stack, boxes):
    """float64 [N, T]; an empty box gives NaN."""
    st = np.asarray(stack, dtype=np.float64)
    out = np.full((len(boxes), st.shape[0]), np.nan)
    for i, (z0, z1, y0, y1, x0, x1) in enumerate(np.asarray(boxes)):
        if z1 > z0 and y1 > y0 and x1 > x0:
            out[i] = st[:, z0:z1, y0:y1, x0:x1].reshape(st.shape[0], -1).mean(1)
    return out


def select_positive(x, k=-1):
    """(k-th smallest positive element, number of positives); k = -1: the lower median."""
    pos = np.sort(np.asarray(x, dtype=F)[np.asarray(x) > 0].ravel())
    if k < 0:
        k = (len(pos) - 1) // 2
    return (pos[k] if k < len(pos) else F(np.nan)), len(pos)


def filter_data(data, k=10):
    return np.convolve(np.asarray(data, dtype=np.float64), np.ones(k) / k, mode="same")


def norm_data(data, filt=10):
    d = np.asarray(data, dtype=np.float64) * 1.0
    if filt != 0:
        d = filter_data(d, filt)
    lo, hi = np.min(d), np.max(d)
    return (d - lo) / (hi if hi != 0 else 1), hi - lo


def corr_coeff(stack_gt, stack_pred, coords, r12, r3, start_plane_offset=-25 // 2, minmax_ths=50, filter_width=10):
    """(correlation coefficients, data-frame values [rows, 6 + T], data-frame index) of CWFA.py:240-337."""
    g = np.asarray(stack_gt, dtype=F)
    p = np.asarray(stack_pred, dtype=F)
    g, p = g / g.max(), p / p.max()
    boxes = roi_boxes(coords, g.shape, r12, r3, start_plane_offset)
    tg, tp = roi_means(g, boxes), roi_means(p, boxes)
    median = select_positive(g)[0]
    ccs, rows, index = [], [], []
    need, halvings = int(len(coords) * 0.2), 0
    while len(ccs) <= need and halvings < 5:
        img_ths = F(median) * F(minmax_ths)
        for i, (x, y, z) in enumerate(coords):
            width = min(filter_width, int(boxes[i, 1] - boxes[i, 0]))
            sg, rng = norm_data(tg[i], width)
            if rng < img_ths:
                continue
            sp, _ = norm_data(tp[i], width)
            cc = 0 if (sg.max() == 0 or sp.max() == 0) else np.corrcoef(sg, sp)[0][1]
            ccs.append(cc)
            zz = z + g.shape[1] // 2 + start_plane_offset
            rows.append([i, x, y, zz, cc, 1, *sg])
            rows.append([i, x, y, zz, cc, 0, *sp])
            index += [i, i]
        if len(ccs) <= need:
            minmax_ths /= 2
            halvings += 1
    return ccs, np.asarray(rows, dtype=np.float64).reshape(len(rows), 6 + g.shape[0]), index


def make_stack(seed, T, shape, boxes, act, bg, noise):
    """A [T,D,H,W] fp32 time series for the corr_coeff_3D fixtures, rebuilt in the tests from the few numbers the fixture stores:
    a static background U(0, bg), per-step noise U(0, noise) (numpy's legacy RandomState: a fixed bit stream) and the stored
    activity act[n, t] added over box n.  Only fp32 additions and exact conversions: the same bits everywhere."""
    rs = np.random.RandomState(seed)
    D, H, W = shape
    base = (rs.random_sample((D, H, W)) * bg).astype(F)
    st = np.empty((T, D, H, W), dtype=F)
    for t in range(T):
        v = base + (rs.random_sample((D, H, W)) * noise).astype(F)
        for n, (z0, z1, y0, y1, x0, x1) in enumerate(boxes):
            v[z0:z1, y0:y1, x0:x1] += F(act[n, t])
        st[t] = v
    return st
