#!/usr/bin/env python3
"""Re-generate the results block of DESIGN.md section 9 from profiles/<tag>_* (run after copying fresh GPU results there):
    python tools/refresh_results.py r02_v3"""
import csv, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = sys.argv[1] if len(sys.argv) > 1 else "r02_v3"
P = lambda n: os.path.join(ROOT, "profiles", f"{TAG}_{n}")   # noqa: E731
d = json.load(open(P("bench.json")))
r, r2, dw = d["roofline"], d["roofline_second"], d["roofline_dwt"]
rows = list(csv.DictReader(open(P("bench_kernel_stats.csv"))))
# tools/prof_bench.sh: 10 timed steps + 3 warm-up / selection + 3 runner-up + 3 chain-event passes
steps = 19
tot = sum(float(x["TotalDurationNs"]) for x in rows) / steps / 1e6
short = lambda n: n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:72]   # noqa: E731
lines = ["| `%s` | %.1f | %.2f | %.1f |" % (short(x["Name"]), int(x["Calls"]) / steps, float(x["TotalDurationNs"]) / steps / 1e6,
                                          float(x["Percentage"])) for x in rows[:16]]
rest = sum(float(x["TotalDurationNs"]) for x in rows[16:]) / steps / 1e6
table = ("| kernel | launches / volume | ms / volume | % |\n|---|---|---|---|\n" + "\n".join(lines) +
         "\n| (%d smaller kernels) | | %.2f | %.1f |\n| total | | %.2f | 100 |" % (len(rows) - 16, rest, 100 * rest / tot, tot))
cb = d["cpu_baseline"]
dom_name = r["kernel"].split(" (")[0]                      # bench.py names a split 3x3 family by its exact kernel instantiation
fam_rows = [x for x in rows if dom_name in x["Name"].replace("(anonymous namespace)::", "")]
avg_dom = sum(float(x["TotalDurationNs"]) for x in fam_rows) / max(sum(int(x["Calls"]) for x in fam_rows), 1) / 1e6
r2_rows = [x for x in rows if r2["kernel"].split(" (")[0] in x["Name"].replace("(anonymous namespace)::", "")]
avg_r2 = sum(float(x["TotalDurationNs"]) for x in r2_rows) / max(sum(int(x["Calls"]) for x in r2_rows), 1) / 1e6
others = []
for bt in ("GLOW", "AI1"):
    f = P(f"bench_{bt}.json")
    if os.path.exists(f):
        g = json.load(open(f))
        others.append(f"{bt} {g['value']:.1f} volumes/s ({g['ms_per_step']:.1f} ms; forward NLL {g.get('forward_nll', {}).get('value', float('nan')):.1f})")
fw = d.get("forward_nll", {})
block = f"""<!-- RESULTS:BEGIN (tools/refresh_results.py {TAG}) -->
| {TAG.replace('_', ' ')} (round 3: + split-bf16 Conv3d, BatchNorm statistics in the conv epilogue, composed first layers, merged first convolutions, seven-wave chain kernels) | **{d['value']:.1f}** | {d['ms_per_step']:.2f} | `{r['kernel'].split(' (')[0]}` (the UNet's 3×3 convolutions without a skip add and the merged first convolution of the four condition nets, {r['launches_timed'] // d['steps']} launches per volume, {100 * r['share_of_conv_time']:.0f} % of the conv time) | {r['algorithmic_tflops']:.0f} algorithmic = {r['achieved']:.0f} issued of 2500 bf16: **{r['frac']:.2f}** | in-path chain {dw['achieved']:.0f} ({dw['frac']:.2f}); largest level {dw['largest_level']['GBps']:.0f} ({dw['largest_level']['GBps'] / 8000:.2f}) |

Same line: runner-up `{r2['kernel'].split(' (')[0]}` {r2['algorithmic_tflops']:.0f} TF/s algorithmic, frac **{r2['frac']:.2f}** ({1e3 * r2['avg_launch_ms']:.1f} µs per launch, 60 launches per volume); plain fp32 MFMA kernels (`fp32_mfma`) {d['fp32_mfma']['value']:.1f} volumes/s; bf16 configuration (`bf16`, BASELINE configs[4]) {d['bf16']['value']:.1f}; forward NLL (configs[3], batch 4 per GPU) {fw.get('value', float('nan')):.1f} volumes/s with its chain at {fw.get('chain_fwd', {}).get('frac', float('nan')):.2f} of the HBM peak; training iteration {d['experiment_train_step']['value']:.2f} volumes/s.  Other block types (`bench.py --block-type`, `profiles/{TAG}_bench_<type>.json`): {'; '.join(others)}.  Standalone wavelet kernels (not launched by the path): four inverse depth-Haar levels {dw['standalone_haar']['achieved']:.0f} GB/s ({dw['standalone_haar']['frac']:.2f}); one-pass 2×2×2 Haar tile {dw['haar3d_tile']['achieved']:.0f} GB/s ({dw['haar3d_tile']['frac']:.2f}).

CPU baseline (oracle, torch CPU): {cb['value']:.4f} volumes/s on {cb['cores']} threads of {cb.get('cpu_model', '?')} ({cb['sample']}) — GPU/CPU = {d['value'] / cb['value']:.0f}×; reported for context, the roofline fraction is the figure of merit.

Dominant kernel traffic (`profiles/{TAG}_pmc_traffic.json`): {(r['traffic'] or 0) / 1e6:.0f} MB per launch HBM-side (FETCH_SIZE×2 + WRITE_SIZE) vs {r['algorithmic_bytes_per_launch'] / 1e6:.0f} MB algorithmic (input once + output once) -- 805 MB before the XCD-aware block order: what is left is the first read of an input tile by the XCD that owns it plus the 10/8 × 34/32 halo where it misses that L2; the layer kernel {(r2['traffic'] or 0) / 1e6:.0f} MB vs {r2['algorithmic_bytes_per_launch'] / 1e6:.0f} MB.  `avg_launch_ms` of `{dom_name}`: {r['avg_launch_ms']:.3f} (HIP events inside bench.py's timed region) vs {avg_dom:.3f} (rocprofv3 `AverageNs` of the same kernel name over the whole profiled run); of `{r2['kernel'].split(' (')[0]}` (all map-layout instantiations): {r2['avg_launch_ms']:.4f} vs {avg_r2:.4f}.

Per-kernel time per volume (rocprofv3 `--kernel-trace --stats` over `bench.py --steps 10 --warmup 3 --full --no-cpu-baseline --no-experiment`, `profiles/{TAG}_bench_kernel_stats.csv`; {steps} volumes in the trace):
{table}
<!-- RESULTS:END -->"""
p = os.path.join(ROOT, "DESIGN.md")
s = open(p).read()
s = re.sub(r"<!-- RESULTS:BEGIN.*?<!-- RESULTS:END -->", lambda m: block, s, flags=re.S)
open(p, "w").write(s)
print("DESIGN.md section 9 refreshed:", round(d["value"], 2), "vol/s")
