#!/bin/bash
# c3 shape, ns per ant-step against the number of environments in the handle (Infinity Cache capacity effect), steady state
R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R
for e in ${ENVS:-384 512 640 768 896 1024 1280 1536 2048}; do
python bench.py --full --envs $e --no-cpu-baseline --no-explicit-sweep --repeats 2 --steps 400 2>/dev/null | python3 -c "
import sys, json; d=json.loads(sys.stdin.read()); k=d['roofline']['kernel_ms']; n=$e*512
print('envs %4d  ms/step %.4f  ns/ant-step %.4f  perceive ns/ant %.4f  update_move ns/ant %.4f' % ($e, d['ms_per_step'], d['ms_per_step']*1e6/n, k['k_perceive']*1e6/n, k['k_update_move']*1e6/n))"
done
