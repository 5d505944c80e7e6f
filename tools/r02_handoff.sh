#!/bin/bash
# GPU: new columnar hand-off tests + bench leg + kernel stats
set -x
R=$PWD; O=$(realpath -m "${1:?usage: bash tools/r02_handoff.sh OUTDIR}"); mkdir -p $O
timeout 900 python -m pytest tests/test_gpu_columns.py tests/test_gpu_rowbinary.py -m gpu -x -q > $O/tests.log 2>&1; tail -5 $O/tests.log
timeout 300 python bench.py --full --steps 3 --warmup 1 --prime 2 --legs handoff --no-cpu-baseline > $O/bench.json 2> $O/bench.err; tail -c 1500 $O/bench.json
cd /tmp && export TMPDIR=/tmp
timeout 300 rocprofv3 --kernel-trace --stats -d $O/prof -o h -- python $R/bench.py --full --steps 2 --warmup 1 --prime 2 --legs handoff --no-cpu-baseline > /dev/null 2>&1
cd $R; find $O/prof -name "*kernel_stats*" | head -1 | xargs -I{} head -25 {}
