#!/bin/bash
# rocprofv3 kernel stats of the default bench (run on the GPU box): tools/prof_bench.sh <tag> [rows]
# The trace and the bench log land in $OUT_DIR (default: bench_out/ in the repo root).
R=$(cd "$(dirname "$0")/.." && pwd)
O=${OUT_DIR:-$R/bench_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_$1
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$1 -o p -- python3 $R/bench.py --steps 10 --warmup 3 --full --no-cpu-baseline --no-experiment > $O/bench_$1.log 2>&1
grep -o '"value": [0-9.]*\|"ms_per_step": [0-9.]*' $O/bench_$1.log
python3 - <<PY
import csv
rows=list(csv.DictReader(open("$O/prof_$1/p_kernel_stats.csv")))
for r in rows[:${2:-18}]:
    print(r["Name"].replace("(anonymous namespace)::","")[:96], int(r["Calls"])//13, round(float(r["TotalDurationNs"])/13e6,3), r["Percentage"])
PY
