#!/usr/bin/env python3
"""Time the neuron footprints on the MI355X and write profiles/footprint_time.json.

At 96 x 512 x 512 (the benchmark's volume), chunks of 16 volumes, N = 200 and N = 4096 neurons planted on a lattice (boxes of 600
voxels, disjoint, every shell non-empty), one GPU process:

  * ``NeuronFootprints.update`` of a chunk: the core sums, the shell sums and the accumulation;
  * ``NeuronFootprints.finish(0.5)``: the correlation and the selection;
  * ``extract_traces`` of a chunk with the neuropil shells;
  * the torch-operator form a user would otherwise write for each of the three: a Python loop over the neurons that slices the
    stack (float64 sums of the same quantities; the fill by iterated shifts of the mask until it stops growing);
  * a float4 copy of 1 GiB (``Tensor.copy_``), the yardstick for what a streaming kernel can reach from HBM.

Every form is warmed up; HIP events around windows of calls; the forms alternate inside one process; median (min, max) over the
windows.  Each of the library's records carries its byte floor -- update: per box voxel 4 T' for the chunk and 2 x 36 for the state
in and out, per neuron 4 T' for each core voxel and 5 T' for each voxel of the shell's outer box (value and occupancy byte); finish:
36 + 4 + 4 + 4 per box voxel (sums in, corr out and in, weights out); traces: (4 T' + 4) per box voxel and the shell bytes -- the
time that floor takes at the copy rate measured in the same run, and the form's time as a multiple of it and of the torch form.
    python tools/footprint_time.py [--quick]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_time import device_record, summary, windows      # noqa: E402

SPACING, FIRST, SIGMA = (12, 20, 20), (6, 10, 10), (1.2, 2.0, 2.0)


def lattice(shape, n):
    """n centres (z, y, x) spread evenly over the lattice FIRST + k SPACING inside the volume."""
    import numpy as np
    axes = [np.arange(f, s - f + 1, d) for f, s, d in zip(FIRST, shape, SPACING)]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    assert len(grid) >= n, (len(grid), n)
    return grid[np.linspace(0, len(grid) - 1, n).astype(np.int64)]


def plant(vols, centres, gen):
    """Add a Gaussian blob with a random amplitude per time step at every centre: footprints of a realistic size come out."""
    import torch
    dz, dy, dx = (torch.arange(-r, r, device="cuda", dtype=torch.float32) for r in (3, 5, 5))
    blob = torch.exp(-0.5 * ((dz[:, None, None] / SIGMA[0]) ** 2 + (dy[None, :, None] / SIGMA[1]) ** 2 + (dx[None, None, :] / SIGMA[2]) ** 2))
    amp = 4.0 * torch.rand(len(centres), vols.shape[0], device="cuda", generator=gen)
    for n, (z, y, x) in enumerate(centres.tolist()):
        vols[:, z - 3:z + 3, y - 5:y + 5, x - 5:x + 5] += amp[n][:, None, None, None] * blob


def torch_forms(vols, g):
    """The three passes as a user would write them with torch operators: a Python loop over the neurons."""
    import torch
    sl = lambda b: (slice(None), slice(int(b[0]), int(b[1])), slice(int(b[2]), int(b[3])), slice(int(b[4]), int(b[5])))
    occ = g.occupancy.bool()
    masks = []
    for o, i in zip(g.shell_outer, g.shell_inner):
        m = ~occ[sl(o)[1:]]
        m[int(i[0] - o[0]):int(i[1] - o[0]), int(i[2] - o[2]):int(i[3] - o[2]), int(i[4] - o[4]):int(i[5] - o[4])] = False
        masks.append(m)
    core_masks = []
    for b, c in zip(g.boxes, g.cores):
        m = torch.zeros(int(b[1] - b[0]), int(b[3] - b[2]), int(b[5] - b[4]), dtype=torch.bool, device="cuda")
        m[int(c[0] - b[0]):int(c[1] - b[0]), int(c[2] - b[2]):int(c[3] - b[2]), int(c[4] - b[4]):int(c[5] - b[4])] = True
        core_masks.append(m)
    sums = {}

    def update():
        for n in range(g.N):
            X = vols[sl(g.boxes[n])].double()
            c = vols[sl(g.cores[n])].double().sum((1, 2, 3))
            u = (vols[sl(g.shell_outer[n])].double() * masks[n]).sum((1, 2, 3))
            d, e, gg = X[1:] - X[0], (c[1:] - c[0])[:, None, None, None], (u[1:] - u[0])[:, None, None, None]
            sums[n] = (d.sum(0), (d * d).sum(0), (d * e).sum(0), (d * gg).sum(0), e.sum(), (e * e).sum(), gg.sum(), (gg * gg).sum(), (e * gg).sum())

    def finish(thr=0.5):
        T = float(vols.shape[0])
        out = []
        for n in range(g.N):
            s1, s2, sc, su, e1, e2, g1, g2, eg = sums[n]
            vi, ve, vg = (s2 - s1 * s1 / T).clamp_min(0), (e2 - e1 * e1 / T).clamp_min(0), (g2 - g1 * g1 / T).clamp_min(0)
            rie, rig, reg = (sc - s1 * e1 / T) / (vi * ve).sqrt(), (su - s1 * g1 / T) / (vi * vg).sqrt(), (eg - e1 * g1 / T) / (ve * vg).sqrt()
            r = ((rie - rig * reg) / ((1 - rig * rig) * (1 - reg * reg)).sqrt()).nan_to_num(0.0)
            above = r >= thr
            cur = above & core_masks[n]
            while True:
                grown = cur.clone()
                grown[1:] |= cur[:-1]
                grown[:-1] |= cur[1:]
                grown[:, 1:] |= cur[:, :-1]
                grown[:, :-1] |= cur[:, 1:]
                grown[:, :, 1:] |= cur[:, :, :-1]
                grown[:, :, :-1] |= cur[:, :, 1:]
                grown &= above
                if torch.equal(grown, cur):
                    break
                cur = grown
            out.append(torch.where(cur, r, 0.0))
        return out

    def traces(weights, alpha=0.7):
        rows = []
        for n in range(g.N):
            F = (vols[sl(g.boxes[n])].double() * weights[n]).sum((1, 2, 3)) / weights[n].sum()
            Fnp = (vols[sl(g.shell_outer[n])].double() * masks[n]).sum((1, 2, 3)) / masks[n].sum()
            rows.append(F - alpha * Fnp)
        return torch.stack(rows)

    return update, finish, traces


def measure(quick):
    import numpy as np
    import torch
    from cwfa_amd import CWFA
    D, H, W = (24, 128, 128) if quick else (96, 512, 512)
    shape, chunk = (D, H, W), 16
    gen = torch.Generator(device="cuda").manual_seed(5)
    n_copy = (1 << 24) if quick else (1 << 28)
    src, dst = torch.rand(n_copy, device="cuda", generator=gen), torch.empty(n_copy, device="cuda")
    shift = D // 2 + (-25 // 2)
    res = {}
    for N in ((20, 64) if quick else (200, 4096)):
        centres = lattice(shape, N)
        vols = torch.rand(chunk, D, H, W, device="cuda", generator=gen)
        plant(vols, centres, gen)
        coords = [[int(x), int(y), int(z) - shift] for z, y, x in centres]
        nf = CWFA.NeuronFootprints(coords, shape, "cuda").update(vols)
        g = nf.geometry
        fp = nf.finish(0.5)
        t_update, t_finish, t_traces = torch_forms(vols, g)
        t_update()
        weights = t_finish()
        V, outer = g.V, int(np.prod(g.shell_outer[:, 1::2] - g.shell_outer[:, 0::2], axis=1).sum())
        cores = int(np.prod(g.cores[:, 1::2] - g.cores[:, 0::2], axis=1).sum())
        nbytes = {"update": V * (4 * chunk + 72) + 4 * chunk * cores + 5 * chunk * outer, "finish": 48 * V,
                  "extract_traces": V * (4 * chunk + 4) + 5 * chunk * outer, "float4_copy": 8 * n_copy}
        fns = {"update": lambda: nf.update(vols), "finish": lambda: nf.finish(0.5),
               "extract_traces": lambda: CWFA.extract_traces(vols, fp, g), "float4_copy": lambda: dst.copy_(src)}
        ms = windows(fns, 3 if quick else 7, 1 if quick else 2, 1 if quick else 2)
        slow = {"torch_update": t_update, "torch_finish": t_finish, "torch_extract_traces": lambda: t_traces(weights)}
        ms.update(windows(slow, 2 if N > 1000 else 3, 1, 1))
        r = {k: summary(v, nbytes.get(k)) for k, v in ms.items()}
        copy_rate = r["float4_copy"]["GBps"]
        for k in ("update", "finish", "extract_traces"):
            r[k]["floor_ms_at_measured_copy_rate"] = round(nbytes[k] / copy_rate / 1e6, 5)
            r[k]["multiple_of_floor"] = round(r[k]["ms"] / r[k]["floor_ms_at_measured_copy_rate"], 1)
            r[k]["torch_form_over_this"] = round(r["torch_" + k]["ms"] / r[k]["ms"], 1)
        sizes = fp.sizes.cpu().numpy()
        r["config"] = {"neurons": N, "state_voxels": V, "state_bytes": 36 * V + 56 * N, "shell_outer_voxels": outer,
                       "footprint_sizes_min_median_max": [int(sizes.min()), float(np.median(sizes)), int(sizes.max())],
                       "samples_in_the_state_when_finish_was_timed": nf.count}
        res[f"N{N}"] = r
        del vols, nf, fp, weights
    res["config"] = {"volume": [D, H, W], "chunk": chunk, "volumes": "uniform random plus a Gaussian blob of random amplitude per neuron",
                     "copy_elements": n_copy, "lattice_spacing": list(SPACING)}
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "footprint_time.py measures on the MI355X; there is no CPU path"
    quick = "--quick" in sys.argv
    rec = {"workload": "neuron footprints: update, finish, extract_traces, and the torch-operator loop over neurons for each",
           "protocol": "ms per call = median (min, max) over windows of HIP-event time / calls, the forms alternating in one process",
           "box": device_record(), "footprints": measure(quick)}
    out = os.path.join(ROOT, "profiles", "footprint_time_quick.json" if quick else "footprint_time.json")
    if os.environ.get("CWFA_PROFILE_OUT"):
        out = os.path.join(os.environ["CWFA_PROFILE_OUT"], os.path.basename(out))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["footprints"]))


if __name__ == "__main__":
    main()
