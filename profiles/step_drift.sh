#!/bin/bash
# How does the step time move as the episode unfolds (ants leave the anthill: colder gathers, more newly
# explored cells)?  40 consecutive regions of 50 steps each from step 0 (no ageing), product path.
R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R
for act in ${ACT_PATHS:-meta}; do
  python bench.py --full --act-path $act --no-cpu-baseline --no-explicit-sweep --age 0 --warmup 0 --steps 2000 --repeats 40 ${BENCH_ARGS} 2>/dev/null | python3 -c "
import sys, json; d=json.loads(sys.stdin.read()); print('$act', d['config']['kernels']); print(' '.join('%.3f' % x for x in d['ms_per_step_regions'])); print(d['roofline']['kernel_ms'])"
done
