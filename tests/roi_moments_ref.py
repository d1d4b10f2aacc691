"""float64 restatement of the exact covariance of ROI means under the posterior of a CAT pyramid, over the
stage dictionaries of tests/posterior_ref.py.

A pyramid is a list of steps in EXECUTION order (coarsest first); a step is ``(stages, shape)`` with ``shape = (B, C, H, W)`` of its
coefficients.  Step i of S has level m = S - i (m = 1: the finest), and C * 2^m is the depth D of the final volume for every step.
The detail v[c, y, x] of level m has variance z_var * exp(a[c, y, x]) (a: the travelling sum of posterior_ref.chain_inv_var), is
independent of every other detail, and enters the final depths [c 2^m, (c + 1) 2^m) at (y, x) with weight +2^(-m/2) on the first
half of that block and -2^(-m/2) on the second.  For boxes r = (z0, z1, y0, y1, x0, x1), half-open, of cnt_r voxels:

    Cov(mean_r1, mean_r2) = z_var / (cnt_r1 cnt_r2) * sum_m 2^-m * sum_c q_r1,m(c) q_r2,m(c) * sum_{(y,x) in both footprints} exp(a_m[c,y,x])

with q_r,m(c) = (depths of [z0, z1) in the first half of block c) - (depths in its second half)."""
import numpy as np
import torch

import posterior_ref as R


def q_table(z0, z1, m, C):
    """int64 [C]: q of the depth range [z0, z1) for every block of level m."""
    size, half = 1 << m, 1 << (m - 1)
    q = np.zeros(C, dtype=np.int64)
    for c in range(C):
        lo = c * size
        first = max(0, min(z1, lo + half) - max(z0, lo))
        second = max(0, min(z1, lo + size) - max(z0, lo + half))
        q[c] = first - second
    return q


def travelling_sum(stages, shape):
    """a <- gather_k(a) - 2 s_k from a = 0: float64 numpy [B, C, H, W]."""
    a = torch.zeros(tuple(shape), dtype=torch.float64)
    for st in stages:
        if st.get("perm") is not None:
            a = a.index_select(st["axis"], st["perm"].to(torch.long))
        s = R.stage_s(st)
        if s is not None:
            a = a - 2.0 * s
    return a.numpy()


def _count(b):
    return max(0, int(b[1]) - int(b[0])) * max(0, int(b[3]) - int(b[2])) * max(0, int(b[5]) - int(b[4]))


def _pairs(boxes, pairs):
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 6)
    if pairs is None:
        pairs = np.repeat(np.arange(len(boxes))[:, None], 2, 1)
    return boxes, np.asarray(pairs, dtype=np.int64).reshape(-1, 2)


def step_term(stages, shape, m, z_var, boxes, pairs=None):
    """One step's term for every pair: (value [B, P], sum of the absolute terms [B, P]), float64.  A pair with an empty box is NaN."""
    boxes, pairs = _pairs(boxes, pairs)
    B, C, H, W = shape
    e = np.exp(travelling_sum(stages, shape))
    val, mag = np.zeros((B, len(pairs))), np.zeros((B, len(pairs)))
    for p, (r1, r2) in enumerate(pairs):
        b1, b2 = boxes[r1], boxes[r2]
        n1, n2 = _count(b1), _count(b2)
        if n1 == 0 or n2 == 0:
            val[:, p] = mag[:, p] = np.nan
            continue
        ya, yb, xa, xb = max(b1[2], b2[2]), min(b1[3], b2[3]), max(b1[4], b2[4]), min(b1[5], b2[5])
        if yb <= ya or xb <= xa:
            continue
        qq = q_table(b1[0], b1[1], m, C) * q_table(b2[0], b2[1], m, C)
        foot = e[:, :, ya:yb, xa:xb].sum(axis=(2, 3))                      # [B, C]
        w = z_var * 2.0 ** -m / (n1 * n2)
        val[:, p] = w * (foot * qq).sum(1)
        mag[:, p] = w * (foot * np.abs(qq)).sum(1)
    return val, mag


def roi_cov(steps, z_var, boxes, pairs=None):
    """The covariance of every pair over a whole pyramid: (value [B, P], sum of the absolute terms [B, P])."""
    S = len(steps)
    val = mag = 0.0
    for i, (stages, shape) in enumerate(steps):
        v, a = step_term(stages, shape, S - i, z_var, boxes, pairs)
        val, mag = val + v, mag + a
    return val, mag


def box_catalogue(D, H, W):
    """The boxes and pairs the fixture and the tests share (D >= 6, H >= 3, W >= 5).  Boxes: 0 one voxel; 1 a depth range that holds
    whole pairs and a whole 4-block plus ragged depths ([3, 9) where D >= 12, else [1, D): a block of four cannot have both ends
    ragged below that); 2 the whole depth range; 3 clipped at the volume's edge (it ends at D, H and W); 4 empty; 5, 6 overlapping
    with a positive covariance; 7, 8 the same footprint on the two halves of the 4-block [0, 4): negative; 9, 10 disjoint
    footprints.  Pairs: (5, 6) +, (7, 8) -, (9, 10) exactly 0, (1, 5) mixed, (0, 4) with the empty box: NaN, (2, 5) with the
    whole-depth box: exactly 0."""
    z1 = (3, 9) if D >= 12 else (1, D)
    boxes = np.array([
        [3, 4, 1, 2, 2, 3],
        [z1[0], z1[1], 0, 2, 1, 4],
        [0, D, 0, 3, 1, 3],
        [D - 3, D, H - 2, H, W - 3, W],
        [2, 5, 1, 1, 0, 4],
        [0, 3, 0, 2, 0, 3],
        [1, 3, 1, 3, 1, 4],
        [0, 2, 0, 2, 0, 2],
        [2, 4, 0, 2, 0, 2],
        [2, 5, 0, 1, 0, 2],
        [2, 5, 2, 3, 3, 5],
    ], dtype=np.int32)
    pairs = np.array([[5, 6], [7, 8], [9, 10], [1, 5], [0, 4], [2, 5]], dtype=np.int32)
    return boxes, pairs


def haar_synthesis_weights(D, levels):
    """[levels][D, D // 2^m]: column c of level m holds the weight of v_m[c] at every final depth (+-2^(-m/2) on block c)."""
    out = []
    for m in range(1, levels + 1):
        Wm = np.zeros((D, D >> m))
        for c in range(D >> m):
            lo, half = c << m, 1 << (m - 1)
            Wm[lo:lo + half, c] = 2.0 ** (-m / 2)
            Wm[lo + half:lo + 2 * half, c] = -(2.0 ** (-m / 2))
        out.append(Wm)
    return out
