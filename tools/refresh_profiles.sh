#!/bin/bash
# Everything profiles/<round>/ holds, re-made on the GPU box (from the repo root), in parts that each fit one gpurun call:
#   tools/refresh_profiles.sh 1   full bench line of the default workload + kernel trace / PMC passes of the three 4096^2 workloads
#   tools/refresh_profiles.sh 2   the 8192^2 workloads + the full bench lines (no micro-benches) of every workload
#   tools/refresh_profiles.sh 3   K2/K3 micro-benches, ICP search, SQ counters of the chain kernel (tools/prof_round_micro.sh)
# The full bench lines land in $QS_BENCH_OUT/<round>/ (default bench_out/<round>/), the profiles where tools/prof_round.sh and
# tools/prof_round_micro.sh put them; copy what is to be judged into profiles/<round>/.
R=${QS_PROF_ROUND:-r03}
B=${QS_BENCH_OUT:-bench_out}/$R
mkdir -p $B
case "$1" in
1)
  python3 bench.py --full > $B/bench_c1_default_run.json 2> $B/bench_c1_default_run.err; echo "default rc=$?"
  bash tools/prof_round.sh c1_4096 && echo c1_4096 ok
  bash tools/prof_round.sh c3_4096 --workload c3 && echo c3_4096 ok
  bash tools/prof_round.sh adv_4096 --workload adv && echo adv_4096 ok
  ;;
2)
  bash tools/prof_round.sh c1_8192 --grid 8192 && echo c1_8192 ok
  bash tools/prof_round.sh c3_8192 --workload c3 --grid 8192 && echo c3_8192 ok
  bash tools/prof_round.sh adv_8192 --workload adv --grid 8192 && echo adv_8192 ok
  for wl in c3 adv; do python3 bench.py --workload $wl --full --no-micro > $B/bench_$wl.json 2> $B/bench_$wl.err; echo "$wl rc=$?"; done
  for wl in c1 c3 adv; do python3 bench.py --workload $wl --grid 8192 --full --no-micro > $B/bench_${wl}_8192.json 2> $B/bench_${wl}_8192.err; echo "$wl 8192 rc=$?"; done
  ;;
3)
  bash tools/prof_round_micro.sh && echo micro ok
  ;;
esac
