"""Restatement of the accelerated Richardson-Lucy loop in plain torch operators, dtype-parametric, on top of
tests/deconv_ref.py: with ``accelerate=False`` it is ``deconv_ref.xlfm_deconv`` operator for operator (bit-equal in float32), in
float64 it is the yardstick of tests/test_gpu_accel_deconv.py.

Statement (Biggs & Andrews 1997): the padded object holds a prediction y_k, x_0 = y_0 = ones;
    x_{k+1} = y_k * back_projection(clamped ratio(y_k))          the reference's iteration, quirks kept, applied to y_k
    g_k     = x_{k+1} - y_k
    alpha   = sum(g_k g_{k-1}) / sum(g_{k-1}^2)                  float64 sums over all depths; clamped to [0, alpha_max]; 0 without a
                                                                 previous step, with a zero denominator or a non-finite quotient
    y_{k+1} = max(x_{k+1} + alpha (x_{k+1} - x_k), 0)            three operations of the working dtype
The trace is the Poisson negative log-likelihood sum(est - img log(est + 1e-8)) in float64 of every forward projection; with ``tol``
the loop ends after the iteration at which, every ``check_every`` iterations, (previous checked - this) / |this| < tol."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from deconv_ref import CDTYPE, shift


def alpha_of(num, den, alpha_max):
    """The clamped quotient of two Python floats; 0 where it does not exist."""
    if den == 0 or not math.isfinite(den) or not math.isfinite(num):
        return 0.0
    q = num / den
    return min(max(q, 0.0), float(alpha_max)) if math.isfinite(q) else 0.0


def poisson_nll(img, est):
    img, est = img.double(), est.double()
    return float((est - img * torch.log(est + 1e-8)).sum())


def xlfm_deconv_accel(OTF, img, nIt, ObjSize, ROIsize, n_split_fourier=1, mult=10, dtype=torch.float32, accelerate=True, alpha_max=0.999,
                      tol=None, check_every=5):
    """(x [1, D, obj, obj], ImgEst [1, 1, F, F], padSize, padSizeImg, iterations run, trace, alphas)."""
    cd = CDTYPE[dtype]
    OTF = OTF.to(cd)
    D, Fs = OTF.shape[1], OTF.shape[2]
    step = D if n_split_fourier == 1 else n_split_fourier
    if OTF.ndim == 4:
        OTF = torch.cat((OTF.unsqueeze(-1), (torch.real(OTF) - 1j * torch.imag(OTF)).unsqueeze(-1)), dim=4)
    OTFt, OTF = OTF[..., 1].clone(), OTF[..., 0].clone()
    padSize = 2 * [(Fs - ObjSize[0]) // 2] + 2 * [(Fs - ObjSize[1]) // 2]
    padSizeImg = 2 * [(Fs - img.shape[2]) // 2] + 2 * [(Fs - img.shape[3]) // 2]
    ImgExp = F.pad(img.to(dtype), padSizeImg)
    X = torch.ones(1, D, ObjSize[0], ObjSize[1], dtype=dtype, device=img.device)        # x_k
    Y = X.clone()                                                                        # y_k
    g_prev = None
    ImgEst = 0 * ImgExp.clone()
    done, trace, alphas, checked = 0, [], [], None
    for ii in range(nIt):
        ImgEst *= 0.0
        ObjTemp = F.pad(Y, padSize)
        for jj in range(0, D, step):
            sl = slice(jj, min(jj + step, D))
            ImgEst += F.relu(shift(torch.fft.irfft2(torch.fft.rfft2(ObjTemp[:, sl]) * OTF[:, sl]))).sum(1).unsqueeze(1)
        Tmp = ImgExp / (ImgEst + 1e-8)
        if Tmp[Tmp != 0].numel() > 0:
            Tmp.clamp_(0.0, Tmp[Tmp != 0].median() * mult)
        if torch.isnan(Tmp).any():
            break
        trace.append(poisson_nll(ImgExp, ImgEst))
        stop = False
        if tol is not None and (ii + 1) % check_every == 0:
            stop = checked is not None and (checked - trace[-1]) / abs(trace[-1]) < tol
            checked = trace[-1]
        Xn = torch.empty_like(X)
        for jj in range(0, D, step):
            sl = slice(jj, min(jj + step, D))
            back = shift(torch.fft.irfft2(torch.fft.rfft2(Tmp) * OTFt[:, sl]))
            Xn[:, sl] = F.pad(ObjTemp[:, sl] * back, [-p for p in padSize])
        done += 1
        if accelerate:
            g = Xn - Y
            a = 0.0 if g_prev is None else alpha_of(float((g.double() * g_prev.double()).sum()), float((g_prev.double() ** 2).sum()), alpha_max)
            alphas.append(a)
            Y = torch.clamp(Xn + torch.tensor(a, dtype=dtype) * (Xn - X), min=0.0)
            g_prev = g
        else:
            Y = Xn
        X = Xn
        if stop:
            break
    X = X.clone()
    X[:, 0:D // 2 - ROIsize[2] // 2] = 0
    X[:, D // 2 + ROIsize[2] // 2:] = 0
    return X, ImgEst, padSize, padSizeImg, done, trace, alphas


# ---------------------------------------------------------------------------------------------- the synthetic problem
def synthetic_problem(seed=0, D=6, obj=16, psf=32, dtype=torch.float64):
    """(OTF complex [1, D, F, F // 2 + 1], img [1, 1, psf, psf]) with F = obj + psf: a five-spot lenslet-like PSF (a centre and four
    satellites whose distance from it grows with depth, so the pattern shears; Gaussian spots that widen away from the middle depth;
    every depth normalised), a sparse object, its forward projection plus a background, Poisson-noised from ``seed``."""
    rng = np.random.default_rng(seed)
    Fs = obj + psf
    yy, xx = np.mgrid[0:psf, 0:psf].astype(np.float64)
    c = (psf - 1) / 2
    P = np.zeros((1, D, psf, psf))
    for z in range(D):
        dz = z - (D - 1) / 2
        r, sig = 7.0 + 1.2 * dz, 0.9 + 0.25 * abs(dz)
        for oy, ox in ((0, 0), (r, 0.3 * dz), (-r, -0.3 * dz), (0.3 * dz, r), (-0.3 * dz, -r)):
            P[0, z] += np.exp(-((yy - c - oy) ** 2 + (xx - c - ox) ** 2) / (2 * sig ** 2))
        P[0, z] /= P[0, z].sum()
    vol = np.where(rng.random((1, D, obj, obj)) > 0.93, rng.random((1, D, obj, obj)) * 400 + 100, 0.0)
    pad = lambda a: np.pad(a, ((0, 0), (0, 0), ((Fs - a.shape[2] + 1) // 2, (Fs - a.shape[2]) // 2), ((Fs - a.shape[3] + 1) // 2, (Fs - a.shape[3]) // 2)))
    otf = torch.fft.rfft2(torch.from_numpy(pad(P)))
    full = shift(torch.fft.irfft2(torch.fft.rfft2(torch.from_numpy(pad(vol))) * otf)).sum(1, keepdim=True).clamp(min=0)
    o = (Fs - psf) // 2
    clean = full[:, :, o:o + psf, o:o + psf].numpy() + 2.0
    img = rng.poisson(clean).astype(np.float64)
    return otf.to(CDTYPE[dtype]), torch.from_numpy(img).to(dtype)
