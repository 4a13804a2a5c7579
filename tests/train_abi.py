"""What the CPU-side checks of the four flat trainers' C-ABI entries share (test_linear_agent_abi_cpu.py's training half,
test_explore_train_abi_cpu.py, test_joint_train_abi_cpu.py, test_rework_train_abi_cpu.py): antsrl_<entry>_grad / _step /
_apply take one argument order behind the net's own leading arguments, so one `Kind` calls them from keywords and one
body checks a refusal.  The cases are data: the lists below are those of the three entries whose limit on B is an
UNSUPPORTED one; the linear file, which differs in small ways, keeps its own in front of pointer_cases()."""
from abi_fakes import FAKE, INVALID, ODD, ODD4, UNSUPPORTED

#: the replay arrays, in the order every entry takes them behind its net
ARRAYS = ("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones")


class Kind:
    """One trainer's entries, called from keywords with a NULL stream.

    entry: "exptrain", ...; net: the names of the net's pointers in _grad and _step (adam_m and adam_v go behind them in
    _step); lead: keywords -> the leading argument (n_features, or the shape); apply_net: what _apply takes in front of
    adam_m, names of keywords ("lead": the leading argument); defaults: B and what else the kind sets (F or shape, a
    workspace of its own); step_defaults: what _step alone has another default for."""

    def __init__(self, entry, net, lead, apply_net, defaults, step_defaults=()):
        self.entry, self.n_net, self.ptrs, self.lead, self.apply_net = entry, len(net), tuple(net) + ARRAYS, lead, apply_net
        self.defaults, self.step_defaults = dict(defaults), dict(step_defaults)

    def who(self, stage):
        return ("%s_%s" % (self.entry, stage)).encode()

    def _call(self, lib, stage, kw, args, defaults=()):
        a = dict({n: FAKE for n in self.ptrs}, n_rows=1000, idx=FAKE, discount=0.5, grads=FAKE, loss=FAKE, work=FAKE, m=FAKE,
                 v=FAKE, step=1, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)
        a.update(self.defaults, **dict(defaults))
        a.update(kw)
        a["lead"] = self.lead(a)
        return getattr(lib, "antsrl_%s_%s" % (self.entry, stage))(*[a[n] for n in args], None)

    def grad(self, lib, **kw):
        return self._call(lib, "grad", kw, ("lead",) + self.ptrs + ("n_rows", "idx", "B", "discount", "grads", "loss", "work"))

    def step(self, lib, **kw):
        return self._call(lib, "step", kw, ("lead",) + self.ptrs[:self.n_net] + ("m", "v") + self.ptrs[self.n_net:]
                          + ("n_rows", "idx", "B", "discount", "step", "lr", "beta1", "beta2", "eps", "grads", "loss", "work"),
                          self.step_defaults)

    def apply(self, lib, **kw):
        return self._call(lib, "apply", kw, self.apply_net + ("m", "v", "grads", "step", "lr", "beta1", "beta2", "eps"))

    def check(self, stages, lib, kw, code, msg):
        """Every stage of `stages` refuses `kw` with `code`, and says `msg` and its own name."""
        for stage in stages:
            assert getattr(self, stage)(lib, **kw) == code, (stage, kw)
            err = lib.antsrl_last_error()
            assert msg in err and self.who(stage) in err, (stage, kw, err)

    def check_grad_needs_grads(self, lib):
        self.check(("grad",), lib, dict(grads=None), INVALID, b"grads is required")
        # (step with grads NULL is valid: checked on the GPU, where it may launch)


def pointer_cases(ptrs):
    """Each of `ptrs` NULL, then each misaligned (dones is a byte array: no alignment to miss)."""
    return [({n: None}, INVALID, n.encode() + b" is required") for n in ptrs] + \
        [({n: ODD}, INVALID, n.encode() + b" must be") for n in ptrs if n != "dones"]


def batch_cases(net_cases, kind):
    """_grad's and _step's: the kind's own cases of its leading argument, B against 65536 rows, the minibatch's
    arguments for the kind's default B, then the pointers."""
    B = kind.defaults["B"]
    return net_cases + [
        (dict(B=0), INVALID, b"B must be"), (dict(B=65537), UNSUPPORTED, b"65536"),
        (dict(n_rows=0), INVALID, b"n_rows"), (dict(idx=None, B=B, n_rows=B - 1), INVALID, b"without idx"),
        (dict(idx=ODD4), INVALID, b"idx must be 8-byte"), (dict(grads=ODD), INVALID, b"grads must be 4-byte"),
        (dict(loss=None), INVALID, b"loss is required"), (dict(loss=ODD), INVALID, b"loss must be 4-byte"),
        (dict(work=None), INVALID, b"workspace is required"), (dict(work=ODD4), INVALID, b"workspace must be 256-byte"),
        (dict(discount=float("nan")), INVALID, b"discount is NaN"), (dict(actions=ODD4), INVALID, b"actions must be 8-byte"),
    ] + pointer_cases(kind.ptrs)


#: n_features of the 32-wide nets, as _grad, _step and _apply refuse it
FEATURE_CASES = [(dict(F=0), INVALID, b"n_features"), (dict(F=1023), UNSUPPORTED, b"n_features + 2")]

#: antsrl_exptrain_sizes' and antsrl_jointtrain_sizes' refusals: F, B, code, message
SIZES_REFUSALS = [(0, 256, INVALID, b"n_features"), (-3, 256, INVALID, b"n_features"), (1023, 256, UNSUPPORTED, b"n_features + 2"),
                  (294, 0, INVALID, b"B must be"), (294, -1, INVALID, b"B must be"), (294, 65537, UNSUPPORTED, b"65536"),
                  (294, 1 << 40, UNSUPPORTED, b"65536")]

#: _step's Adam arguments (all INVALID); the first six are _apply's too
ADAM_CASES = [(dict(step=0), b"step must be >= 1"), (dict(lr=-1.0), b"lr"), (dict(lr=float("nan")), b"lr"),
              (dict(beta1=1.0), b"beta1"), (dict(beta2=-0.1), b"beta1, beta2"), (dict(eps=0.0), b"eps"),
              (dict(m=None), b"adam_m is required"), (dict(v=ODD), b"adam_v must be 4-byte")]


def apply_cases(net_cases):
    """_apply's: the kind's own cases of its leading argument, the four pointers, Adam's scalars."""
    return net_cases + [(dict(model=None), INVALID, b"model is required"), (dict(grads=None), INVALID, b"grads is required"),
                        (dict(m=ODD), INVALID, b"adam_m must be"), (dict(v=None), INVALID, b"adam_v is required")] + \
        [(kw, INVALID, msg) for kw, msg in ADAM_CASES[:6]]
