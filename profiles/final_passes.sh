#!/bin/bash
# The round's profile set (one gpurun call per configuration keeps each call short):
#   CONFIGS="c3" bash profiles/final_passes.sh
# kernel trace + stats of a bench run, then the PMC passes (each in its own run, --kernel-trace only).  Every run ages the
# episode by bench.py's default 400 steps first: kernel_stats, the bench line's kernel_ms and the PMC bytes all describe
# the same steady regime.
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
export PROFILE_OUT=${PROFILE_OUT:-$R/profile_out}  # the raw output of every pass (read by summarize.py; pmc_pass.sh writes there too)
O=$PROFILE_OUT; mkdir -p $O
for c in ${CONFIGS:-c3}; do
  cd /tmp
  rm -rf $O/prof_$c
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$c -- \
      python3 $R/bench.py --full --config $c --steps 200 --repeats 2 --no-cpu-baseline --no-explicit-sweep > $O/bench_${c}_rocprof.json 2> $O/prof_$c.err
  tail -c 700 $O/bench_${c}_rocprof.json; echo
  BENCH_ARGS="--config $c" bash $R/profiles/pmc_pass.sh ${c}_fetch FETCH_SIZE | grep "k_perceive\|k_move\|k_update\|k_act\|k_sweep\|k_policy"
  BENCH_ARGS="--config $c" bash $R/profiles/pmc_pass.sh ${c}_write WRITE_SIZE | grep "k_perceive\|k_move\|k_update\|k_act\|k_sweep\|k_policy"
done
