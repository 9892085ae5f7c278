#!/bin/bash
# round-3 bench lines + rocprofv3 of bench.py itself (the command the roofline object comes from).  usage (on an MI355X): tools/profile_round.sh OUTDIR
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$(realpath -m "${1:?usage: tools/profile_round.sh OUTDIR}"); mkdir -p $O
cd $R
timeout -k 10 400 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/r03_bench_C2_driver.json 2> $O/r03_bench_C2_driver.err
timeout -k 10 400 python bench.py --full > $O/r03_bench_C2.json 2> $O/r03_bench_C2.err
timeout -k 10 300 python bench.py --full --config C1 --steps 8000 --warmup 200 --no-cpu-baseline > $O/r03_bench_C1.json 2> $O/r03_bench_C1.err
timeout -k 10 300 python bench.py --full --config C3 --steps 300 --warmup 20 --no-cpu-baseline > $O/r03_bench_C3.json 2> $O/r03_bench_C3.err
timeout -k 10 300 python bench.py --full --config C5 --steps 300 --warmup 20 --no-cpu-baseline > $O/r03_bench_C5.json 2> $O/r03_bench_C5.err
cd /tmp && export TMPDIR=/tmp
rm -rf $O/r03_bench_prof
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/r03_bench_prof -- python3 $R/bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --no-dropin > $O/r03_bench_C2_driver_under_rocprof.json 2> $O/r03_bench_prof.err
cd $R; for f in $O/r03_bench_C2_driver.json $O/r03_bench_C2.json $O/r03_bench_C1.json $O/r03_bench_C3.json $O/r03_bench_C5.json $O/r03_bench_C2_driver_under_rocprof.json; do python - $f <<'PY'
import json, sys
j = json.load(open(sys.argv[1])); r = j["roofline"]
print(sys.argv[1].split("/")[-1], round(j["value"] / 1e6, 1), "M/s", r["kernel_short"], "frac", round(r["frac"], 3), "mem", r.get("memory_side_frac"), "period us", round(r["avg_launch_period_us"], 2),
      "epoch", (j.get("epoch") or {}).get("cold", {}).get("value"), (j.get("epoch") or {}).get("replay", {}).get("value"), "long", (j.get("long_stream") or {}).get("value"))
PY
done
