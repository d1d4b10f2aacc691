"""Write the deconvolution fixtures tests/golden/g25_deconv_*.npz: seeded inputs, arguments and the outputs of the REFERENCE's own
XLFMDeconv, fft_conv_split, fft_conv and load_PSF_OTF on the CPU (imported by oracle.make_golden's recipe), beside the outputs of
the float64 restatement (tests/deconv_ref.py) and dev_ref = max|ref - f64| / max|f64| per recorded tensor.  Inputs, arguments and
recorded outputs only.  Run from the repository root:  python tools/make_deconv_golden.py

The generator asserts what the tests rely on: the fp32 restatement equals the reference bit for bit, dev_ref < 2e-6, and at least
two depths of every deconvolved volume are zeroed by the region of interest."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.make_golden import dump, import_reference  # noqa: E402

import deconv_ref as R  # noqa: E402

# name: (depths, PSF, object, iterations, ROI depths, n_split_fourier values, image offset, 5-D OTF)
DECONV = {"i": (5, 24, 12, 4, 2, (1,), 0.0, False), "ii": (5, 24, 12, 4, 2, (1,), -1.0, False),
          "iii": (5, 32, 14, 6, 2, (1, 2), 0.0, False), "iv": (7, 32, 16, 20, 4, (1,), 0.0, True)}
SPLIT = {"odd_h": ((2, 4, 13, 12), 24), "odd_h2": ((2, 4, 11, 12), 24), "even": ((2, 4, 14, 14), 32)}


def npy(t):
    return t.detach().cpu().numpy().copy()


def dev_of(ref, f64):
    return np.float64((ref.double() - f64).abs().max() / f64.abs().max())


def sparse_psf(torch, g, D, n):
    p = torch.rand(1, D, n, n, generator=g) ** 6
    return p / p.sum((2, 3), keepdim=True)


def sparse_volume(torch, g, shape, scale):
    return torch.where(torch.rand(shape, generator=g) < 0.85, torch.zeros(()), torch.rand(shape, generator=g)) * scale


def main():
    import torch
    import_reference()
    import utils as RU
    RU.tqdm = lambda it, **kw: it
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(2525)

    for name, (D, P, obj, nIt, roi, splits, offset, five) in DECONV.items():
        psf = sparse_psf(torch, g, D, P)
        vol = sparse_volume(torch, g, (1, D, obj, obj), 25.0)
        img, OTF = RU.fft_conv_split(vol, psf, torch.tensor([P, P]), n_split=1)
        img = img + 0.05 * img.mean() * torch.randn(img.shape, generator=g) + offset
        img[:, :, :3] = 0
        if five:
            OTF = torch.cat((OTF.unsqueeze(-1), (torch.real(OTF) - 1j * torch.imag(OTF)).unsqueeze(-1)), 4)
        arrs = dict(OTF=npy(OTF), img=npy(img), nIt=np.int64(nIt), ObjSize=np.array([obj, obj]), PSFShape=np.array([P, P]),
                    ROIsize=np.array([obj, obj, roi]), splits=np.array(splits), mult=np.int64(10))
        if offset:
            print("  negative fraction", float((img < 0).float().mean()), "image mean", float(img.mean()))
            assert float((img < 0).float().mean()) > 0.02
        for ns in splits:
            out = RU.XLFMDeconv(OTF.clone(), img.clone(), nIt, ObjSize=[obj, obj], PSFShape=[P, P], ROIsize=[obj, obj, roi],
                                n_split_fourier=ns, device="cpu")
            assert len(out) == 6 and out[1] == 0 and out[3] == []
            r32 = R.xlfm_deconv(OTF, img, nIt, [obj, obj], [obj, obj, roi], ns, 10, torch.float32)
            assert r32[4] == nIt
            assert torch.equal(r32[0], out[0]) and torch.equal(r32[1], out[2]), f"{name}: the fp32 restatement is not the reference"
            assert r32[2] == out[4] and r32[3] == out[5]
            r64 = R.xlfm_deconv(OTF, img, nIt, [obj, obj], [obj, obj, roi], ns, 10, torch.float64)
            zeroed = [z for z in range(D) if not out[0][0, z].any()]
            assert len(zeroed) >= 2 and out[0].abs().max() > 0, (name, zeroed)
            k = f"n{ns}/"
            arrs[k + "vol"], arrs[k + "est"] = npy(out[0]), npy(out[2])
            arrs[k + "vol64"], arrs[k + "est64"] = npy(r64[0]), npy(r64[1])
            arrs[k + "dev_vol"], arrs[k + "dev_est"] = dev_of(out[0], r64[0]), dev_of(out[2], r64[1])
            assert arrs[k + "dev_vol"] < 2e-6 and arrs[k + "dev_est"] < 2e-6, (name, ns, arrs[k + "dev_vol"], arrs[k + "dev_est"])
            arrs[k + "tuple_len"], arrs[k + "zeroed"] = np.int64(len(out)), np.array(zeroed)
            arrs[k + "padSize"], arrs[k + "padSizeImg"] = np.array(out[4]), np.array(out[5])
            print(f"  {name} n_split_fourier={ns}: dev_vol {arrs[k + 'dev_vol']:.2e} dev_est {arrs[k + 'dev_est']:.2e} zeroed {zeroed}")
        dump(f"g25_deconv_rl_{name}", **arrs)

    for name, (shape, P) in SPLIT.items():
        vol = sparse_volume(torch, g, shape, 10.0)
        psf = sparse_psf(torch, g, shape[1], P)
        ps = torch.tensor([P, P])
        img2, otf2 = RU.fft_conv_split(vol, psf, ps, n_split=2)
        img1 = RU.fft_conv_split(vol, otf2, ps, n_split=1, B_precomputed=True)
        full = (shape[2] + P, shape[3] + P)
        fc, fc_otf = RU.fft_conv(vol, psf, torch.tensor(full))
        a32, o32 = R.fft_conv_split(vol, psf, ps, 2)
        b32 = R.fft_conv_split(vol, otf2, ps, 1, True)[0]
        c32 = R.fft_conv(vol, psf, full)
        assert torch.equal(a32, img2) and torch.equal(o32, otf2) and torch.equal(b32, img1), f"{name}: the fp32 restatement is not the reference"
        assert torch.equal(c32[0], fc) and torch.equal(c32[1], fc_otf)
        a64, o64 = R.fft_conv_split(vol, psf, ps, 2, dtype=torch.float64)
        b64 = R.fft_conv_split(vol, o64, ps, 1, True, dtype=torch.float64)[0]
        c64 = R.fft_conv(vol, psf, full, dtype=torch.float64)[0]
        arrs = dict(vol=npy(vol), psf=npy(psf), psf_shape=np.array([P, P]), img2=npy(img2), otf2=npy(otf2), img1=npy(img1), conv=npy(fc),
                    img2_64=npy(a64), otf2_64=npy(o64), img1_64=npy(b64), conv64=npy(c64))
        arrs["dev_img2"], arrs["dev_img1"], arrs["dev_conv"] = dev_of(img2, a64), dev_of(img1, b64), dev_of(fc, c64)
        arrs["dev_otf"] = np.float64((otf2.to(torch.complex128) - o64).abs().max() / o64.abs().max())
        assert max(arrs["dev_img2"], arrs["dev_img1"], arrs["dev_conv"], arrs["dev_otf"]) < 2e-6
        print(f"  {name}: dev img2 {arrs['dev_img2']:.2e} img1 {arrs['dev_img1']:.2e} conv {arrs['dev_conv']:.2e} otf {arrs['dev_otf']:.2e}")
        dump(f"g25_deconv_split_{name}", **arrs)

    # load_PSF / load_PSF_OTF behind a stand-in for the file reader: a non-square stack of 9 depths, 4 of them used
    raw = (torch.rand(26, 24, 9, generator=g) ** 6).numpy()
    RU.loadmat = lambda filename: {"PSF": raw}
    psf_in = RU.load_PSF("none", 4)
    otf, shape = RU.load_PSF_OTF("none", [12, 12, 4], n_split=2)
    otf5, _ = RU.load_PSF_OTF("none", [12, 12, 4], n_split=2, compute_OTF=True)
    o64 = R.fft_conv_split(torch.zeros(1, 4, 12, 12), psf_in.double(), shape, 2, dtype=torch.float64)[1]
    arrs = dict(raw=np.ascontiguousarray(raw.transpose(2, 0, 1))[None], psf=npy(psf_in), otf=npy(otf), otf5=npy(otf5), psf_shape=npy(shape),
                vol_size=np.array([12, 12, 4]), otf64=npy(o64))
    arrs["dev_otf"] = np.float64((otf.to(torch.complex128) - o64).abs().max() / o64.abs().max())
    assert arrs["dev_otf"] < 2e-6
    dump("g25_deconv_psf", **arrs)


if __name__ == "__main__":
    main()
