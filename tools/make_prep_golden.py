"""Write the data preparation fixtures tests/golden/g22_prep_*.npz: seeded inputs, arguments and the outputs of the REFERENCE's own
load_process_volume, crop_volume_center, fast_quantile, load_XLFM_data, pad_img_to_min, center_crop, the frame clean-up of
XLFMDatasetFull.__init__ and the ConcatDataset methods on the CPU (imported by oracle.make_golden's recipe).  Inputs, arguments,
outputs and raised-exception flags only.  Run from the repository root:  python tools/make_prep_golden.py

The generator asserts the conditions the tests rely on (a discrete step must not be able to hide an error): in every crossing
fast_quantile case the walk stops with at least 2 counts to spare on both sides; one case does not cross; at least 1 % of the
volume elements lie exactly on an interior bin edge; at least one element equals the top edge."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.make_golden import dump, import_reference  # noqa: E402

import prep_ref as R  # noqa: E402


def npy(t):
    return t.detach().cpu().numpy().copy()            # a copy: the reference goes on writing into some of these tensors


def make_volumes(torch, g, shape, top):
    """fp16-grid volumes: about 70 % exact zeros, the rest on multiples of 8 up to 1000 (exact in fp16), `top` elements above."""
    u = torch.rand(shape, generator=g)
    lev = torch.randint(1, 126, shape, generator=g).float() * 8
    v = torch.where(u < 0.7, torch.zeros(()), lev)
    flat = v.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:top]
    flat[idx] = 1200.0 + 16 * torch.arange(top, dtype=torch.float32)
    return v.half()


def main():
    import torch
    import_reference()
    import utils as RU                                   # the reference's modules (import_reference put them on the path)
    import XLFMDataset as RX
    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(2222)

    # ------------------------------------------------------------------ volumes: load_process_volume / crop_volume_center
    vols = {"a": (make_volumes(torch, g, (3, 10, 37, 41), 12), [32, 36, 10]), "b": (make_volumes(torch, g, (2, 6, 32, 32), 5), [32, 32, 6])}
    arrs, cases = {}, []
    calls = {"none": dict(volume_ths=[], norm=None), "two": dict(volume_ths=[24.0, 1000.0], norm=None),
             "float": dict(volume_ths=0.05, norm=None), "max": dict(volume_ths=0.1, norm="max")}
    for vn, (v, size) in vols.items():
        arrs[f"vol_{vn}"], arrs[f"size_{vn}"] = npy(v), np.array(size, dtype=np.int64)
        arrs[f"crop_{vn}"] = npy(RU.crop_volume_center(v, [1, size[2], size[0], size[1]]))
        for cn, kw in calls.items():
            out = RU.load_process_volume(v.clone(), size, **kw)
            assert out.dtype == torch.float16
            arrs[f"{vn}/{cn}"] = npy(out)
            cases.append(f"{vn}/{cn}")
    v3 = make_volumes(torch, g, (9, 8, 6), 2)                       # a single 3-D volume in the two permuted channel orders
    arrs["vol3"] = npy(v3)
    arrs["vol3/xyz"] = npy(RU.load_process_volume(v3.clone(), [7, 8, 6], volume_ths=[24.0, 1000.0], norm=None, channel_order="xyz"))
    arrs["vol3/yxz"] = npy(RU.load_process_volume(v3.clone(), [8, 5, 6], volume_ths=[24.0, 1000.0], norm=None, channel_order="yxz"))
    for name, kw in (("std", dict(norm="std")), ("resize", dict(resize=True))):
        try:
            RU.load_process_volume(vols["b"][0].clone(), [32, 32, 6], volume_ths=0.1, **kw)
            arrs[f"raised_{name}"] = np.int64(0)
        except NameError:                                           # resize_volume is not defined in the reference
            arrs[f"raised_{name}"] = np.int64(1)
    arrs["cases"] = np.array(cases)
    dump("g22_prep_volumes", **arrs)

    # ------------------------------------------------------------------ frames: the clean-up of XLFMDatasetFull.__init__
    raw = (torch.rand(3, 45, 52, generator=g) * 3000).numpy().astype(np.float32)
    raw[0, 3, 7], raw[1, 20, 30], raw[2, 44, 51] = np.nan, np.inf, -np.inf
    raw[0, 10, 10], raw[1, 2, 50], raw[2, 22, 26] = -17.5, 61234.0, 50000.5
    raw[0, 22, 26], raw[1, 22, 27] = 2049.0, 2051.0                 # ties of the fp16 rounding (even and odd neighbours)
    RX.imread = lambda path, maxworkers=None, key=None: raw[key].copy()
    RX.get_lenslet_centers = lambda filename: torch.zeros(1, 2, dtype=torch.int32)
    RX.tqdm = lambda it, **kw: it
    arrs = dict(raw=raw)
    for S in (40, 44):
        ds = RX.XLFMDatasetFull("none", "none", img_shape=[S, S], images_to_use=[0, 1, 2], load_vols=False)
        arrs[f"views_{S}"] = npy(ds.stacked_views)
        img = torch.from_numpy(raw[0])
        padded = RX.pad_img_to_min(img)
        arrs[f"padded_shape"] = np.array(padded.shape, dtype=np.int64)
        arrs[f"center_crop_{S}"] = npy(RX.center_crop(padded[None, None], [S, S]))[0, 0]
    dump("g22_prep_frames", **arrs)

    # ------------------------------------------------------------------ fast_quantile on prepared volumes
    prepared = RU.load_process_volume(vols["a"][0].clone(), vols["a"][1], volume_ths=[24.0, 1000.0], norm=None).float()
    arrs = dict(x=npy(prepared))
    h, edges = torch.histogram(prepared, bins=10000)
    flat = npy(prepared).ravel()
    on_edge = np.isin(flat, npy(edges)[1:-1]).mean()
    assert on_edge >= 0.01, on_edge
    assert (flat == npy(edges)[-1]).sum() >= 1
    arrs["counts"], arrs["edges"] = npy(h).astype(np.int64), npy(edges)
    qcases, crossing = [], 0
    for quant in (0.5, 0.9, 0.97, 0.99999):
        val = RU.fast_quantile(prepared, quant)
        e, n_bin, crossed, above, below = R.quantile_walk(npy(h), npy(edges), quant)
        assert np.float32(val) == e, (quant, float(val), e)
        if crossed:
            assert above >= 2 and below >= 2, (quant, above, below)
            crossing += 1
        else:
            assert n_bin == 9999
        arrs[f"q{quant}/value"], arrs[f"q{quant}/crossed"] = np.float32(val), np.int64(crossed)
        qcases.append(quant)
    assert crossing >= 2 and not arrs["q0.99999/crossed"]
    arrs["quants"] = np.array(qcases, dtype=np.float64)
    dump("g22_prep_quantile", **arrs)

    # ------------------------------------------------------------------ load_XLFM_data with a stand-in dataset class
    views = {n: torch.from_numpy(R.prep_frames((torch.rand(len(vols[n][0]), 45, 52, generator=g) * 3000).numpy(), 40, 40)) for n in vols}
    current = {}

    class StandIn:
        def __init__(self, *a, **kw):
            self.vols, self.stacked_views = current["vols"].clone(), current["views"].clone()

        def __len__(self):
            return self.vols.shape[0]

        standarize = RX.XLFMDatasetFull.standarize
        standarize_sample = staticmethod(RX.XLFMDatasetFull.standarize_sample)

    RU.XLFMDatasetFull = StandIn
    configs = {"two_q": dict(volume_ths=[24.0, 1000.0], volume_quantiles=[0.0, 0.9], img_ths=[0.3, 1.0], norm=None),
               "float_noq": dict(volume_ths=0.05, volume_quantiles=[0.0, 1], img_ths=[0.1, 1.0], norm=None),
               "max_q": dict(volume_ths=0.1, volume_quantiles=[0.0, 0.97], img_ths=[0.5, 1.0], norm="max")}
    arrs = {f"views_{n}": npy(views[n]) for n in vols}
    datasets = {}
    for cn, kw in configs.items():
        for n in vols:
            current["vols"], current["views"] = vols[n][0], views[n]
            ds = RU.load_XLFM_data("none", "none", vols[n][1], [40, 40], None, 10, n, **kw)
            assert ds.vols.dtype == torch.float32
            arrs[f"{cn}/{n}/vols"], arrs[f"{cn}/{n}/views"] = npy(ds.vols), npy(ds.stacked_views)
            assert 0.02 < float((ds.stacked_views == 0).float().mean()) < 0.98
            datasets[(cn, n)] = ds
    arrs["configs"] = np.array(list(configs))
    dump("g22_prep_pipeline", **arrs)

    # ------------------------------------------------------------------ ConcatDataset on the prepared datasets
    for cn in ("two_q",):
        pair = [datasets[(cn, "b")], StandIn.__new__(StandIn)]
        pair[1].vols, pair[1].stacked_views = datasets[(cn, "b")].vols.flip(0) * 0.5, datasets[(cn, "b")].stacked_views.flip(0) * 0.25
        both = RX.ConcatDataset(*pair)
        arrs = {"vols_0": npy(pair[0].vols), "vols_1": npy(pair[1].vols), "views_0": npy(pair[0].stacked_views), "views_1": npy(pair[1].stacked_views)}
        arrs["stats"] = np.array([float(s) for s in both.get_statistics()], dtype=np.float32)
        arrs["mean0"], arrs["std0"] = npy(both.mean(0)), npy(both.std(0))
        arrs["max"] = np.array([float(m) for m in both.get_max()], dtype=np.float32)
        arrs["len"] = np.int64(len(both))
        one = RX.ConcatDataset(pair[0])
        arrs["stats_one"] = np.array([float(s) for s in one.get_statistics()], dtype=np.float32)
        both.normalize_datasets()
        for k in (0, 1):
            arrs[f"norm/vols_{k}"], arrs[f"norm/views_{k}"] = npy(pair[k].vols), npy(pair[k].stacked_views)
        stats = both.get_statistics()
        arrs["norm/stats"] = np.array([float(s) for s in stats], dtype=np.float32)
        both.standarize_datasets(stats)
        for k in (0, 1):
            arrs[f"stand/vols_{k}"], arrs[f"stand/views_{k}"] = npy(pair[k].vols), npy(pair[k].stacked_views)
        dump("g22_prep_concat", **arrs)


if __name__ == "__main__":
    main()
