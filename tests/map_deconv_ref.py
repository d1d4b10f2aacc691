"""Restatement of MAP Richardson-Lucy in plain torch operators, dtype-parametric, on top of
tests/accel_deconv_ref.py: with no prior and no ``init`` it is ``accel_deconv_ref.xlfm_deconv_accel`` operator for operator (bit-equal
in float32), in float64 it is the yardstick of tests/test_gpu_map_deconv.py.

Statement: a Poisson likelihood and an independent Gaussian prior N(mu, sigma^2) per voxel, w = weight / sigma^2.  With a the plain
update of a voxel (y * back projection), the EM M-step maximises -x + a log x - w / 2 (x - mu)^2, the positive root of
w x^2 + c x - a = 0 with c = 1 - w mu, in the form that only adds terms of one sign:
    r = sqrt(max(c c + 4 (w a), 0))
    x = 2 a / (c + r)        where c > 0
    x = (r - c) / (2 w)      elsewhere (c <= 0 implies w mu >= 1, so w > 0)
The maximum with 0 only acts where a < 0 (rounding noise of a back projection).  The trace is the objective: the Poisson negative
log-likelihood of the projection of y_k plus sum(w / 2 (y_k - mu)^2), in float64."""
import numpy as np
import torch
import torch.nn.functional as F

from accel_deconv_ref import alpha_of, poisson_nll
from deconv_ref import CDTYPE, shift


def m_step(a, mu, w):
    """The M-step on tensors of one dtype, one rounding per operator.  The branch not taken may hold 0 / 0; ``where`` drops it."""
    c = 1 - w * mu
    r = torch.sqrt(torch.clamp(c * c + 4 * (w * a), min=0))
    return torch.where(c > 0, 2 * a / (c + r), (r - c) / (2 * w))


def penalty(y, mu, w):
    """sum(w / 2 (y - mu)^2) in float64 of tensors of any dtype."""
    d = y.double() - mu.double()
    return float((0.5 * w.double() * (d * d)).sum())


def xlfm_deconv_map(OTF, img, nIt, ObjSize, ROIsize, n_split_fourier=1, mult=10, dtype=torch.float32, accelerate=False, alpha_max=0.999,
                    tol=None, check_every=5, prior_mean=None, prior_std=None, prior_weight=1.0, init=None, keep=None):
    """(x [1, D, obj, obj], ImgEst [1, 1, F, F], padSize, padSizeImg, iterations run, trace, alphas).  ``keep``: a dict that receives
    ``"a"``, the plain update y * back projection of the last iteration run, before the M-step."""
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
    X = torch.ones(1, D, ObjSize[0], ObjSize[1], dtype=dtype, device=img.device) if init is None else init.to(dtype).clone()   # x_k
    Y = X.clone()                                                                        # y_k
    prior = prior_mean is not None
    if prior:
        mu, sd = prior_mean.to(dtype), prior_std.to(dtype)
        w = torch.tensor(prior_weight, dtype=dtype) / (sd * sd)
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
        trace.append(poisson_nll(ImgExp, ImgEst) + penalty(Y, mu, w) if prior else poisson_nll(ImgExp, ImgEst))
        stop = False
        if tol is not None and (ii + 1) % check_every == 0:
            stop = checked is not None and (checked - trace[-1]) / abs(trace[-1]) < tol
            checked = trace[-1]
        Xn = torch.empty_like(X)
        for jj in range(0, D, step):
            sl = slice(jj, min(jj + step, D))
            back = shift(torch.fft.irfft2(torch.fft.rfft2(Tmp) * OTFt[:, sl]))
            a = F.pad(ObjTemp[:, sl] * back, [-p for p in padSize])
            Xn[:, sl] = m_step(a, mu[:, sl], w[:, sl]) if prior else a
            if keep is not None:
                keep.setdefault("a", torch.empty_like(X))[:, sl] = a
        done += 1
        if accelerate:
            g = Xn - Y
            al = 0.0 if g_prev is None else alpha_of(float((g.double() * g_prev.double()).sum()), float((g_prev.double() ** 2).sum()), alpha_max)
            alphas.append(al)
            Y = torch.clamp(Xn + torch.tensor(al, dtype=dtype) * (Xn - X), min=0.0)
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


# ---------------------------------------------------------------------------------------------- the prior of the tests
def prior_recipe(plain64, seed=7):
    """(mu, sigma, start) float32 numpy arrays shaped like ``plain64``, the plain loop's float64 result: with xs its mean,
    mu = xs |N(0, 1)|, sigma = sqrt(xs) exp(U(-1.5, 1.5)), one voxel in ten sigma = +inf, start = max(mu, 1e-3 xs).  w mu >= 1, the
    second branch of the M-step, is |N| >= exp(2 U): about a third of the voxels whatever xs is."""
    rng = np.random.default_rng(seed)
    v = np.asarray(plain64, dtype=np.float64)
    xs = float(v.mean())
    mu = xs * np.abs(rng.standard_normal(v.shape))
    sigma = np.sqrt(xs) * np.exp(rng.uniform(-1.5, 1.5, v.shape))
    sigma[rng.random(v.shape) < 0.1] = np.inf
    mu, sigma = mu.astype(np.float32), sigma.astype(np.float32)
    return mu, sigma, np.maximum(mu, np.float32(1e-3 * xs))
