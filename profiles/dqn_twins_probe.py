"""Fresh LinearTrainers in one process on the same arrays and idx at (294, 65536), compared bit for bit: the instrument behind
DESIGN §7.13's localisation, with more variants than tests/test_gpu_dqn_train_workspace.py's four twins.  The modes alternate
step(), grad() + apply(), step(keep_grads=False), grad() + apply().  After each, the partials, grads, loss, heads and
Adam's state are compared with the first trainer's, and a difference is printed (agent_harness.twin_report: which
workgroups and outputs, their values and ulp distances, and whether the ordered sum of a trainer's own partials gives its
own gradients).  Nothing is asserted.  profiles/dqn_twins_probe.txt is its output on the kernel BEFORE k_lintrain was
limited to one wave per SIMD; profiles/dqn_launch_repeat.py counts such events over hundreds of launches.

Three variants per input set tell a trainer that steps at once after its construction from one whose net is read
first, and both from a launch that is simply repeated:
  at-once       nothing between LinearTrainer(...), its weights and the step (the old test's twin)
  settled       the net is cloned on the device first (four small kernels), as the workspace tests' snapshots do
  same-trainer  ONE trainer, grad() four times: no construction, no allocation and no Adam step between the launches
Input sets: test_step_equals_the_contract's without and with dones, and linear_train_cases' full-F294-B65536, at which the
rotation head's TD error is small by construction and an operand that is off shows large.

    python profiles/dqn_twins_probe.py            # one MI355X; a second of run time"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from agent_harness import linear_snapshot, same_bits, twin_report  # noqa: E402
from agent_harness import random_linear_replay as _random_replay  # noqa: E402

F, N, B = 294, 3000, 65536
MODES = ("step", "grad", "step_no_grads", "grad")
OUTPUTS = ("partials", "grads", "loss", "heads", "adam")


def run(tr, mode, arrays, idx):
    if mode == "grad":
        loss = tr.grad(arrays, idx)
        tr.apply()
        return loss
    return tr.step(arrays, idx, keep_grads=mode == "step")


def input_sets():
    """(name, arrays, idx, a function that builds a fresh trainer) per input set."""
    from antsrl_amd.train import LinearTrainer
    import linear_train_cases as K

    def seeded():
        tr = LinearTrainer(F, "cuda", seed=3 + B % 7)
        tr.target_l3.mul_(0.5)
        return tr
    for with_done in (False, True):
        arrays, g = _random_replay(N, F, B + with_done, with_done)
        yield "with_done %d" % with_done, arrays, torch.randint(0, N, (B,), device="cuda", generator=g), seeded
    case = K.WORKSPACE[K.WORKSPACE_IDS.index("full-F294-B65536")]
    inp = K.inputs(case)

    def loaded():
        tr = LinearTrainer(F, "cuda", discount=case["discount"], state_dict=inp["sd"])
        tr.target_l3.copy_(torch.cat([inp["target"][0].reshape(-1), inp["target"][1]]))
        return tr
    yield case["name"], tuple(a.cuda().contiguous() for a in inp["arrays"]), inp["idx"].cuda(), loaded


def main():
    differed = total = 0
    for name, arrays, idx, fresh in input_sets():
        for variant in ("at-once", "settled", "same-trainer"):
            snaps, modes = [], MODES if variant != "same-trainer" else ("grad_only",) * 4
            tr = fresh() if variant == "same-trainer" else None
            for mode in modes:
                if variant != "same-trainer":
                    tr = fresh()
                if variant == "settled":
                    kept = [t.clone() for t in (tr.policy.w1, tr.policy.b1, tr.heads, tr.target_l3)]  # noqa: F841
                loss = tr.grad(arrays, idx) if mode == "grad_only" else run(tr, mode, arrays, idx)
                s = linear_snapshot(tr, loss, B, grads=mode != "step_no_grads")
                s.update(w1=tr.policy.w1.cpu(), b1=tr.policy.b1.cpu(), target_l3=tr.target_l3.cpu())  # the step writes none of them
                snaps.append(s)
            for i, s in enumerate(snaps[1:], 1):
                inputs = all(same_bits(snaps[0][k], s[k]) for k in ("w1", "b1", "target_l3"))
                bad = [k for k in OUTPUTS if k in s and not same_bits(snaps[0][k], s[k])]
                differed += bool(bad)
                total += 1
                print("%s, %s, trainer %d (%s): inputs %s; %s" % (
                    name, variant, i, modes[i], "equal" if inputs else "DIFFER",
                    "equal bits" if not bad else "DIFFERS in " + ", ".join(bad) + twin_report(snaps[0], s)))
    print("%d of %d comparisons differed" % (differed, total))


if __name__ == "__main__":
    main()
