#!/bin/bash
# one GPU cycle: parity tests, the full bench line, rocprofv3 kernel trace of a shorter full bench run.  usage: tools/gpu_cycle.sh TAG OUTDIR
TAG=${1:-x}
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$(realpath -m "${2:?usage: tools/gpu_cycle.sh TAG OUTDIR}"); mkdir -p $O
cd $R
timeout -k 10 500 python -m pytest tests -m gpu -x -q > $O/test_$TAG.log 2>&1; echo "pytest exit $?" >> $O/test_$TAG.log; tail -4 $O/test_$TAG.log
timeout -k 10 300 python bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err; echo "bench exit $?"; cat $O/bench_$TAG.json; tail -3 $O/bench_$TAG.err
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -- python3 $R/bench.py --full --no-cpu-baseline --steps 300 --warmup 20 > $O/prof_$TAG.log 2>&1; echo "prof exit $?"
head -6 $O/prof_$TAG/*/*_kernel_stats.csv | cut -c1-150
