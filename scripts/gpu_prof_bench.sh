#!/bin/bash
# kernel statistics of the full bench command itself (timed graph replays + the eager roofline rounds): the averages that
# bench.py's roofline objects are checked against
R=${GRAFT_REPO_ROOT:-/root/repo}
T=${1:-bench}
OUT=${OUT:-$R/prof_out}; mkdir -p $OUT
cd /tmp; export TMPDIR=/tmp
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_b -o b -- python $R/bench.py --full --no-cpu-baseline > $OUT/${T}_under_rocprof.json 2> $OUT/${T}_prof.err
find /tmp/prof_b -name '*kernel_stats.csv' -exec cp {} $OUT/${T}_bench_kernel_stats.csv \;
cut -c1-300 $OUT/${T}_under_rocprof.json
head -4 $OUT/${T}_bench_kernel_stats.csv | cut -c1-200
