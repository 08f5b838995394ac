#!/bin/bash
# `rocprofv3 --kernel-trace --stats` of bench.py for the non-default presets (tag $1): one kernel-stats CSV per BASELINE.json configuration.
# Results in $OUT/<tag>_keep/ (default prof_out/, under the repository root; copy into profiles/).
T=${1:-r03r}; R=$(pwd); O=${OUT:-prof_out}
mkdir -p $O/${T}_keep
cd /tmp; export TMPDIR=/tmp
for p in c1 c2 c3 c4 c5; do
  extra=""; [ $p = c5 ] && extra="--steps 1 --warmup 1"; [ $p = c4 ] && extra="--steps 2 --warmup 1"
  timeout 1200 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/${T}_stats_$p -- python3 $R/bench.py --preset $p --full --no-cpu-baseline --presets 0 $extra > $R/$O/${T}_stats_$p.log 2>&1
  f=$(find $R/$O/${T}_stats_$p -name "*kernel_stats.csv" | head -1)
  cp $f $R/$O/${T}_keep/${T}_rocprofv3_kernel_stats_bench_$p.csv
  grep '^{"metric' $R/$O/${T}_stats_$p.log > $R/$O/${T}_keep/${T}_bench_${p}_under_rocprof.json
  head -5 $f | cut -c1-170
done
