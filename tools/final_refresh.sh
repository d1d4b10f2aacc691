#!/bin/bash
# On the GPU box, from the repo root: tools/final_refresh.sh <tag>   (e.g. r02_v3)
# PMC traffic -> full bench line (forward NLL leg, fp32 / bf16 figures, training experiment, cpu_baseline) -> rocprofv3 kernel
# stats of the headline command -> bench lines of the other block types.  Everything lands in $OUT_DIR (default: bench_out/ in
# the repo root); copy what should be judged into profiles/ afterwards (tools/refresh_results.py <tag> then rewrites the results
# block of DESIGN.md).
set -e
T=${1:-r02}
R=$(cd "$(dirname "$0")/.." && pwd)
export OUT_DIR=${OUT_DIR:-$R/bench_out}
O=$OUT_DIR
mkdir -p $O
(cd /tmp && timeout -k 10 500 python3 $R/tools/pmc_traffic.py $O/${T}_pmc_traffic.json > $O/pmc.log 2>&1) || echo "pmc pass failed (see $O/pmc.log)"
[ -s $O/${T}_pmc_traffic.json ] && cp $O/${T}_pmc_traffic.json $R/profiles/${T}_pmc_traffic.json
timeout -k 10 900 python3 $R/bench.py --full > $O/bench_full.log 2> $O/bench_full.err
tail -1 $O/bench_full.log > $O/${T}_bench.json
python3 -c "
import json; d=json.load(open('$O/${T}_bench.json')); r=d['roofline']
print('value', d['value'], 'ms', d['ms_per_step'], 'frac', r['frac'], 'avg_ms', r['avg_launch_ms'], 'traffic', r['traffic'], 'cpu', d.get('cpu_baseline', {}).get('value'), 'dwt', d['roofline_dwt']['frac'], 'fwd', d.get('forward_nll', {}).get('value'))"
$R/tools/prof_bench.sh ${T} 30 > $O/prof_${T}.txt 2>&1
for bt in GLOW AI1; do
  timeout -k 10 300 python3 $R/bench.py --full --block-type $bt --steps 10 --warmup 3 --no-cpu-baseline > $O/${T}_bench_$bt.json 2> $O/bench_$bt.err || echo "$bt failed"
  grep -o '"value": [0-9.]*' $O/${T}_bench_$bt.json | head -1
done
