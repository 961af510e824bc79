#!/bin/bash
# Copy one gpu_evidence.sh run's summaries from $OUT (default bench_out/) into profiles/<round>/
# (tracked): pmc_traffic.json (the file bench.py reads, stamped with the source
# hash), tagged copies of the bench line, kernel-trace stats and summaries.
# Usage: tools/save_evidence.sh <round dir, e.g. profiles/r02> <tag>
set -e
D=$1; T=$2
OUT="${OUT:-bench_out}"  # where gpu_evidence.sh wrote
mkdir -p "$D"
cp $OUT/pmc_traffic.json "$D/pmc_traffic.json"
cp $OUT/pmc_traffic.json "$D/${T}_pmc_traffic.json"
tail -1 $OUT/bench.log > "$D/${T}_bench.json"
cp $OUT/trace_summary.json "$D/${T}_trace_summary.json"
f=$(ls $OUT/prof/*/run_kernel_stats.csv $OUT/prof/run_kernel_stats.csv 2>/dev/null | head -1)
cp "$f" "$D/${T}_kernel_stats.csv"
cp $OUT/pytest_gpu.log "$D/${T}_pytest_gpu.log"
[ -f $OUT/smoke.log ] && cp $OUT/smoke.log "$D/${T}_smoke.log"
echo "saved $T into $D"
