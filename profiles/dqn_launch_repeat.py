"""Do equal launches of the linear trainer's gradient stage give equal bits?  ONE LinearTrainer, grad() launched --launches
times on linear_train_cases' full-F294-B65536 (512 workgroups of k_lintrain, one tile per wave; inputs at which a workgroup
that is off shows large), the workspace read back after each.  Every launch's partials are compared with the per-element
mode over the launches; prints how many launches hold a workgroup that differs and which (launch, workgroup), then the
median time of a grad() by hipEvents.  The instrument behind DESIGN §7.13's counts: run it once per library
(ANTSRL_LIB selects an A/B build) to hold a variant of the kernel against the one in the tree.

    python profiles/dqn_launch_repeat.py [--launches 400]        # one MI355X, a few seconds"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]

import benchlib as BL  # noqa: E402
import linear_train_cases as K  # noqa: E402
import linear_train_ref as L  # noqa: E402


def main():
    from antsrl_amd import _lib
    from antsrl_amd.train import LinearTrainer
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    n = ap.parse_args().launches
    case = K.WORKSPACE[K.WORKSPACE_IDS.index("full-F294-B65536")]
    inp = K.inputs(case)
    B, nb = case["B"], L.blocks(case["B"])
    tr = LinearTrainer(case["F"], "cuda", discount=case["discount"], state_dict=inp["sd"])
    tr.target_l3.copy_(torch.cat([inp["target"][0].reshape(-1), inp["target"][1]]))
    arrays, idx = tuple(a.cuda().contiguous() for a in inp["arrays"]), inp["idx"].cuda()
    torch.cuda.synchronize()
    parts = []
    for _ in range(n):
        tr.grad(arrays, idx)
        parts.append(tr._work.cpu().view(torch.int32)[: nb * L.PART].view(nb, L.PART)[:, :L.OUT].clone())
    bits = torch.stack(parts)                                # [launches, workgroups, outputs], as bit patterns
    bad = (bits != bits.mode(dim=0).values).any(dim=2)       # [launches, workgroups]
    events = [(int(i), int(w)) for i, w in bad.nonzero().tolist()]
    print("library %s: %d of %d launches hold a workgroup whose partials differ from the mode; (launch, workgroup) %s%s"
          % (_lib.LIB_PATH, int(bad.any(1).sum()), n, events[:24], " ..." if len(events) > 24 else ""))
    ms = BL.per_call([lambda: tr.grad(arrays, idx)], 100, 0)[0]  # (the launches above are the warm-up)
    print("grad() at F = %d, B = %d: median %.4f ms over 100" % (case["F"], B, sorted(ms)[50]))


if __name__ == "__main__":
    main()
