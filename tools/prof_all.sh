#!/bin/bash
# rocprof evidence + full bench lines for a list of configs (run on the GPU box):
#   bash tools/prof_all.sh <tag> <cfg> [<cfg> ...]
#   -> the rocprofv3 data of tools/prof_bench.sh (trace, fetch, write) and the `bench.py --full`
#      line $BENCH_OUT/<tag>_bench_<cfg>.json (default bench_out/; tools/fill_traffic.py reads it there)
set -o pipefail
R=$GRAFT_REPO_ROOT
[ -n "$R" ] || R=$(pwd)
TAG=$1; shift
mkdir -p $R/gpurun_out
O=${BENCH_OUT:-$R/bench_out}
mkdir -p $O
for cfg in "$@"; do
  steps=20; [ "$cfg" = synth ] && steps=10; [ "$cfg" = rcv1_stress ] && steps=5
  (cd $R && timeout -k 10 400 python3 bench.py --full --config $cfg --steps $steps --warmup 3 > $O/${TAG}_bench_$cfg.log 2>&1) || { echo "bench $cfg failed"; tail -5 $O/${TAG}_bench_$cfg.log; exit 1; }
  grep '"metric"' $O/${TAG}_bench_$cfg.log > $O/${TAG}_bench_$cfg.json
  python3 $R/tools/ab_line.py "$cfg" $O/${TAG}_bench_$cfg.json
  bash $R/tools/prof_bench.sh ${TAG}_$cfg --config $cfg || exit 1
done
