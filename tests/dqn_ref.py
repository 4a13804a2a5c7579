"""What the restatements of the agents' training steps share (linear_train_ref.py, explore_train_ref.py,
memory_train_ref.py): the replay ring's array names, the unit roundoffs and Higham's gamma, the bfloat16
rounding, a gathered batch as tensors, torch.optim.Adam's single-tensor step over named tensors, a forward error bound
carried through one DQN head to the loss and that head's gradient sums, and the share of a bound an error uses.  CPU only.

A net's own file keeps what is the net's: the two restatements of its step, the bound of its layers in front of the head,
and its cases."""
import numpy as np
import torch

#: the arrays of a replay ring, in the order every `batch` and `arrays` tuple has them
RING = ("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones")
U_BF16 = 2.0 ** -9   # bfloat16's unit roundoff (8 significand bits, round to nearest even)
U_FP32 = 2.0 ** -24  # fp32's unit roundoff


def gamma(n, u=U_FP32):
    """Higham's gamma_n = n u / (1 - n u): n roundings of relative size u compound to at most this."""
    return n * u / (1.0 - n * u)


def bf16(x):
    return torch.as_tensor(x, dtype=torch.float32).to(torch.bfloat16).to(torch.float32)


def as_batch(batch):
    """A gathered batch (RING's order, arrays or tensors) as tensors: rows flattened, fp32, actions int64, dones bool."""
    st, ast, act, rw, nst, nast, dn = batch
    f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)  # noqa: E731
    B = len(rw)
    return (f(st).reshape(B, -1), f(ast).reshape(B, 2), torch.as_tensor(np.asarray(act), dtype=torch.int64), f(rw),
            f(nst).reshape(B, -1), f(nast).reshape(B, 2), torch.as_tensor(np.asarray(dn), dtype=torch.bool))


def gather(arrays, idx):
    return tuple(a[idx].numpy() for a in arrays)


def adam(names, state, grads, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam, single tensor, fp32 per element; the bias corrections in double.  Steps state["sd"][k] for k in
    names from grads[k], with the moments state["m"][k], state["v"][k] and the count state["step"]."""
    state["step"] += 1
    t = state["step"]
    bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
    step_size, bc2_sqrt = np.float32(lr / bc1), np.float32(bc2 ** 0.5)
    for k in names:
        g = grads[k].to(torch.float32)
        m, v = state["m"][k], state["v"][k]
        m.lerp_(g, float(np.float32(1.0 - betas[0])))
        v.mul_(float(np.float32(betas[1]))).addcmul_(g, g, value=float(np.float32(1.0 - betas[1])))
        denom = (v.sqrt() / float(bc2_sqrt)).add_(float(np.float32(eps)))
        state["sd"][k].addcdiv_(m, denom, value=-float(step_size))


def propagate_head(W, b, tw, tb, a, rw, live, discount, h, hn, eh, ehn, own=0.0, elem=0.0, rowsum=0.0, loss_elem=0.0):
    """One head's share of a forward error bound, carried to the loss and the head's gradient sums.  W, b: the head; tw,
    tb: the head the TD target takes its max over; a [B]: the action taken; h, hn the hidden values of the rows and of
    their successors and eh, ehn what they may be off by (float64, [B, 32]).
        e_q  = e_h |W|^T + own ((|h| + e_h) |W|^T + |b|)        own: the head's own sum (0: exact)
        e_y  = discount max_o e_q' (max is 1-Lipschitz);  e_d = e_q[action] + e_y + elem (|q| + |reward| + discount |max q'| + e_q + e_y)
        loss:  sum_b (2 |d| e_d + e_d^2) / (3 B)  +  (rowsum + loss_elem) sum_b (|d| + e_d)^2 / (3 B)
        grad:  sum_b 2 / (3 B) (e_d (|h| + e_h) + |d| e_h)  +  rowsum sum_b 2 / (3 B) (|d| + e_d) (|h| + e_h)
    (weights; h := 1, e_h := 0 for the biases).  Returns (loss bound, weight bound [3, 32], bias bound [3], d [B], e_d [B]):
    d and e_d are what a layer in front of the head carries on."""
    loss, gw, gb, d, ed = propagate_head_grouped(W, b, tw, tb, a, rw, live, discount, h, hn, eh, ehn,
                                                 torch.zeros((len(rw),), dtype=torch.int64),
                                                 torch.tensor([rowsum], dtype=torch.float64), own, elem, loss_elem)
    return float(loss[0]), gw[0], gb[0], d, ed


def propagate_head_grouped(W, b, tw, tb, a, rw, live, discount, h, hn, eh, ehn, group, rowsum, own=0.0, elem=0.0,
                           loss_elem=0.0):
    """propagate_head with the rows summed group by group: group [B] int64 names the sum a row goes into (a workgroup's
    partial, say) and rowsum [G] float64 is the row-sum factor of each.  B in 2 / (3 B) and 1 / (3 B) stays the batch's.
    Returns (loss bound [G], weight bound [G, 3, 32], bias bound [G, 3], d [B], e_d [B])."""
    W, b, tw, tb = W.double(), b.double(), tw.double(), tb.double()
    B, G = len(rw), len(rowsum)
    rows = torch.arange(B)
    q = (h @ W.T + b)[rows, a]
    qn = (hn @ tw.T + tb).max(dim=1).values
    d = q - (rw.double() + discount * qn * live)
    eq = (eh @ W.abs().T + own * ((h.abs() + eh) @ W.abs().T + b.abs()))[rows, a]
    ey = discount * (ehn @ tw.abs().T + own * ((hn.abs() + ehn) @ tw.abs().T + tb.abs())).max(dim=1).values * live
    ed = eq + ey + elem * (q.abs() + rw.double().abs() + discount * qn.abs() * live + eq + ey)

    def sums(per, index, n):  # per [B, ...] -> [n, ...]: the rows of each index added up
        return torch.zeros((n,) + per.shape[1:], dtype=torch.float64).index_add_(0, index, per)
    loss = sums((2 * d.abs() * ed + ed * ed) / (3 * B), group, G) + (rowsum + loss_elem) * sums((d.abs() + ed) ** 2 / (3 * B), group, G)
    c, slot = 2.0 / (3 * B), group * 3 + a  # a gradient row per group and action
    fwd = sums(c * (ed[:, None] * (h.abs() + eh) + d.abs()[:, None] * eh), slot, 3 * G).view(G, 3, 32)
    mag = sums(c * (d.abs() + ed)[:, None] * (h.abs() + eh), slot, 3 * G).view(G, 3, 32)
    gw = fwd + rowsum[:, None, None] * mag
    gb = sums(c * ed, slot, 3 * G).view(G, 3) + rowsum[:, None] * sums(c * (d.abs() + ed), slot, 3 * G).view(G, 3)
    return loss, gw, gb, d, ed


def worst_share(got, want, bound, keys):
    """max over the elements of |got - want| / bound (an element with a zero bound must be equal: inf otherwise)."""
    worst = 0.0
    for k in keys:
        err = (got[k].double() - want[k].double()).abs()
        bd = torch.as_tensor(bound[k], dtype=torch.float64)
        share = torch.where(err == 0, torch.zeros_like(err), err / bd)
        worst = max(worst, float(share.max()))
    return worst
