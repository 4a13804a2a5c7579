"""Builds profiles/memory_train_stages.json from the printed records of the memory trainer's stage and exact tests
(DESIGN §7.7):

    python -m pytest tests/test_memory_train_bounds_cpu.py -s -q > cpu.log
    python -m pytest tests/test_gpu_memory_train_stages.py -m gpu -s -q > gpu.log      (on an MI355X)
    python profiles/memory_train_stages.py cpu.log gpu.log

The shares are |value - float64 stage| / a-priori bound, worst element per launch; nothing in them is read from the
kernels.  A record, not a threshold: the tests assert <= 1."""
import ast
import json
import os
import sys


def main(cpu_log, gpu_log=None):
    out = dict(exact_coverage={}, cpu_restatement_share={}, cpu_defect_factor={}, device_share={})
    for line in open(cpu_log):
        line = line.lstrip(".")
        for tag, key in (("EXACT-COVERAGE ", "exact_coverage"), ("STAGE-CPU-SHARE ", "cpu_restatement_share"),
                         ("STAGE-CPU-DEFECT ", "cpu_defect_factor")):
            if line.startswith(tag):
                name, rest = line[len(tag):].split(" ", 1)
                out[key][name] = ast.literal_eval(rest.strip())
    if gpu_log:
        for line in open(gpu_log):
            if line.startswith("STAGE-GPU-SHARE "):
                rec = json.loads(line[len("STAGE-GPU-SHARE "):])
                out["device_share"][rec["case"]] = rec["shares"]
    fac = [(v, d, c) for c, ds in out["cpu_defect_factor"].items() for d, v in ds.items() if v != "inf"]
    if fac:
        v, d, c = min(fac)
        out["mildest_defect"] = dict(factor_over_bound=v, defect=d, case=c)
    for key in ("cpu_restatement_share", "device_share"):
        stages = {}
        for shares in out[key].values():
            for s, v in shares.items():
                stages[s] = max(stages.get(s, 0.0), v)
        out[key + "_worst_by_launch"] = stages
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "memory_train_stages.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in out if k.endswith("worst_by_launch") or k == "mildest_defect"}, indent=1))


if __name__ == "__main__":
    main(*sys.argv[1:3])
