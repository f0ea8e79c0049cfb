#!/bin/bash
# rocprofv3 kernel stats of one bench step with its side measurements (--full) -> $OUT_DIR/kernel_stats.txt (default prof_out/)
set -u
REPO=$(pwd)
OUT=$REPO/${OUT_DIR:-prof_out}
mkdir -p $OUT
export TMPDIR=/tmp
cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof -o runc -- python $REPO/bench.py --steps 1 --warmup 1 --full --no-cpu-baseline "$@" > $OUT/rocprof_bench.log 2>&1
cd $REPO && python benchmarks/summarize_rocprof.py /tmp/prof $OUT/kernel_stats.txt 60 > /dev/null 2>&1
grep '^{' $OUT/rocprof_bench.log | tail -1 | cut -c1-400
head -40 $OUT/kernel_stats.txt | cut -c1-200
