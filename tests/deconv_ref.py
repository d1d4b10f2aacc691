"""Restatement of the reference's Richardson-Lucy deconvolution (utils.py:449-738) in plain torch operators, dtype-parametric: in
float32 on the CPU it reproduces the reference bit for bit (tools/make_deconv_golden.py asserts that), in float64 it is the yardstick
of the GPU tests.  Runs on any device (tools/deconv_time.py times it on the GPU as the operator-by-operator baseline).

Statement: centred zero pad (ceil in front for fft_conv, equal on both sides for XLFMDeconv), rfft2, product with the transfer
function, irfft2, roll by -ceil(n / 2) on both axes; forward projection relu + depth sum per chunk; ratio img / (est + 1e-8), clamp
to [0, mult * median of the non-zero elements]; back projection with the conjugate transfer function; multiplicative update of the
object's window; the depths outside the region of interest zeroed at the end."""
import numpy as np
import torch
import torch.nn.functional as F

CDTYPE = {torch.float32: torch.complex64, torch.float64: torch.complex128}


def shift(x):
    """batch_fftshift2d_real: out[i] = x[(i + ceil(n / 2)) mod n] on the last two axes."""
    return torch.roll(x, (-((x.shape[-2] + 1) // 2), -((x.shape[-1] + 1) // 2)), (-2, -1))


def pad_centre(A, fh, fw):
    dh, dw = fh - A.shape[2], fw - A.shape[3]
    return F.pad(A, [(dw + 1) // 2, dw // 2, (dh + 1) // 2, dh // 2])


def fft_conv(A, B, full, precomputed=False, dtype=torch.float32):
    """(shifted planes, OTF).  A [Ba, n, h, w]; B the PSF [1, n, ph, pw], or the OTF when ``precomputed``."""
    fh, fw = int(full[0]), int(full[1])
    otf = B.to(CDTYPE[dtype]) if precomputed else torch.fft.rfft2(pad_centre(B.to(dtype), fh, fw))
    return shift(torch.fft.irfft2(torch.fft.rfft2(pad_centre(A.to(dtype), fh, fw)) * otf)), otf


def fft_conv_split(A, B, psf_shape, n_split, precomputed=False, dtype=torch.float32):
    """(image [Ba, 1, ph, pw], OTF [1, D, fh, fw // 2 + 1]): chunks of D // n_split depths, the first n_split of them."""
    D, (ph, pw) = A.shape[1], (int(v) for v in psf_shape)
    fh, fw = A.shape[2] + ph, A.shape[3] + pw
    step = D // n_split
    oy, ox = -((ph - fh) // 2), -((pw - fw) // 2)
    img = torch.zeros(A.shape[0], 1, ph, pw, dtype=dtype, device=A.device)
    otf_out = torch.zeros(1, D, fh, fw // 2 + 1, dtype=CDTYPE[dtype], device=A.device)
    for n in range(n_split):
        sl = slice(n * step, (n + 1) * step)
        cur, otf = fft_conv(A[:, sl], B[:, sl], (fh, fw), precomputed, dtype)
        otf_out[:, sl] = otf
        img += cur[:, :, oy:oy + ph, ox:ox + pw].sum(1).unsqueeze(1).abs()
    return img, otf_out


def xlfm_deconv(OTF, img, nIt, ObjSize, ROIsize, n_split_fourier=1, mult=10, dtype=torch.float32):
    """(ObjRecon [1, D, obj, obj], ImgEst [1, 1, F, F], padSize, padSizeImg, iterations run).  OTF 4-D (conjugate formed here, as the
    reference forms it) or 5-D [.., 2]; img [1, 1, H, W] with a non-zero sum."""
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
    ObjRecon = torch.ones(1, D, ObjSize[0], ObjSize[1], dtype=dtype, device=img.device)
    ImgEst = 0 * ImgExp.clone()
    done = 0
    for ii in range(nIt):
        ImgEst *= 0.0
        ObjTemp = F.pad(ObjRecon, padSize)
        for jj in range(0, D, step):
            sl = slice(jj, min(jj + step, D))
            ImgEst += F.relu(shift(torch.fft.irfft2(torch.fft.rfft2(ObjTemp[:, sl]) * OTF[:, sl]))).sum(1).unsqueeze(1)
        Tmp = ImgExp / (ImgEst + 1e-8)
        if Tmp[Tmp != 0].numel() > 0:
            Tmp.clamp_(0.0, Tmp[Tmp != 0].median() * mult)
        if torch.isnan(Tmp).any():
            break
        for jj in range(0, D, step):
            sl = slice(jj, min(jj + step, D))
            back = shift(torch.fft.irfft2(torch.fft.rfft2(Tmp) * OTFt[:, sl]))
            ObjRecon[:, sl] = F.pad(ObjTemp[:, sl] * back, [-p for p in padSize])
        done += 1
    ObjRecon[:, 0:D // 2 - ROIsize[2] // 2] = 0
    ObjRecon[:, D // 2 + ROIsize[2] // 2:] = 0
    return ObjRecon, ImgEst, padSize, padSizeImg, done


# ---------------------------------------------------------------------------------------------- numpy float64, per kernel
def np_shift_index(n, off=0):
    """Source index of target index i + off under the shift: (i + off + ceil(n / 2)) mod n."""
    return (np.arange(n) + off + (n + 1) // 2) % n


def np_project(p, window=None, pre=None, post=None):
    """float64: (sum over depth [N, Ho, Wo] of the shifted, windowed planes after ``pre``, with ``post``; sum of |terms|)."""
    p = np.asarray(p, dtype=np.float64)
    N, D, H, W = p.shape
    oy, ox, Ho, Wo = (0, 0, H, W) if window is None else window
    rows, cols = np_shift_index(H)[oy:oy + Ho], np_shift_index(W)[ox:ox + Wo]
    t = p[:, :, rows][:, :, :, cols]
    if pre == "relu":
        t = np.maximum(t, 0.0)
    s = t.sum(1)
    return (np.abs(s) if post == "abs" else s), np.abs(t).sum(1)


def np_select_nonzero(x, k=-1):
    """(k-th smallest of the elements != 0 or NaN, their count); k = -1: the lower median."""
    v = np.sort(np.asarray(x).ravel()[np.asarray(x).ravel() != 0])
    if k < 0:
        k = (len(v) - 1) // 2 if len(v) else 0
    return (v[k] if k < len(v) else np.float32(np.nan)), len(v)
