"""The module states a fine-tuning run puts YoloNet in, stated once for the training tests (CPU only; no GPU, no kernel).

A state says which parameters are trainable and how each BatchNorm runs.  It says so three ways that must agree
(tests/test_train_states_host.py asserts it on a CPU YoloNet):

* ``apply(net)`` sets ``requires_grad``, ``.train()`` / ``.eval()`` and, where the state says so, ``momentum``, ``eps`` and
  ``num_batches_tracked`` of its BatchNorms on a YoloNet (``apply_modes(net)``: everything but ``requires_grad``);
* ``trainable(param_name) -> bool`` in tests/train_ref.py's ``param_names``;
* ``bn(prefix) -> (training, momentum, eps, num_batches_tracked_before)`` for a conv_bn_relu prefix (``feature.mlist.0``,
  ``up1.conv``; a trailing ``.bn`` is accepted), for the float64 restatements.

``expected_walk(state, ops)`` restates, from the docstring of yolo_v3_amd/backprop.py and not from its code, which ops the reverse walk
visits under a state and what each must do there."""
from tests import train_ref as T
from tests import yolo_loss_ref as R
from yolo_v3_amd import arch

MOMENTUM, EPS = 0.1, 1e-5                      # nn.BatchNorm2d's defaults, which YoloNet keeps
WALK_KEYS = ("dw", "dx_after", "dcat", "dlow_after", "dtail_after", "res_after")      # the trace keys expected_walk speaks of


def cbr_prefixes():
    """The 72 conv_bn_relu prefixes in the order backprop.graph(net) runs them (reference darknet.py:198-231)."""
    out, pos = ["feature.mlist.0"], 1
    for nb in arch.BACKBONE_BLOCKS:
        out.append("feature.mlist.%d" % pos)
        pos += 1
        for _ in range(nb):
            out += ["feature.mlist.%d.conv1" % pos, "feature.mlist.%d.conv2" % pos]
            pos += 1
    for name, up in (("pre_det1", "up1.conv"), ("pre_det2", "up2.conv"), ("pre_det3", None)):
        out += ["%s.mlist.%d" % (name, i) for i in range(6)]
        if up:
            out.append(up)
    return out


def res_blocks():
    """Prefixes of the residual blocks (``feature.mlist.N`` holding conv1 and conv2)."""
    return sorted({p.rsplit(".", 1)[0] for p in cbr_prefixes() if p.endswith(".conv1")})


def _is_bn_param(name):
    return name.endswith((".bn.weight", ".bn.bias"))


class State:
    """name; trainable: param name -> bool; bn: conv_bn_relu prefix -> (training, momentum, eps, num_batches_tracked_before);
    modes: optional extra call on the net before the BatchNorms are set (a state defined through a parent module's mode)."""

    def __init__(self, name, trainable, bn=None, modes=None):
        self.name, self._trainable, self._bn, self._modes = name, trainable, bn, modes

    def __repr__(self):
        return "State(%s)" % self.name

    def trainable(self, param_name):
        return bool(self._trainable(param_name))

    def bn(self, prefix):
        if prefix.endswith(".bn"):
            prefix = prefix[:-3]
        training, momentum, eps, nbt = self._bn(prefix) if self._bn is not None else (True, MOMENTUM, EPS, 0)
        return bool(training), momentum, float(eps), int(nbt)

    def factor(self, prefix):
        """The weight of the batch in the running-statistics update, as nn.BatchNorm2d computes it."""
        _, momentum, _, nbt = self.bn(prefix)
        return 1.0 / (nbt + 1) if momentum is None else float(momentum)

    def uniform_bn(self):
        """True / False when every BatchNorm runs in that mode with the default settings, else None."""
        s = {self.bn(p) for p in cbr_prefixes()}
        return s.pop()[0] if len(s) == 1 and next(iter(s))[1:] == (MOMENTUM, EPS, 0) else None

    def apply_modes(self, net):
        net.train()
        if self._modes is not None:
            self._modes(net)
        mods = dict(net.named_modules())
        for p in cbr_prefixes():
            training, momentum, eps, nbt = self.bn(p)
            m = mods[p].bn
            m.train(training)
            m.momentum, m.eps = momentum, eps
            m.num_batches_tracked.fill_(nbt)
        return net

    def apply(self, net):
        self.apply_modes(net)
        for n, p in net.named_parameters():
            p.requires_grad_(self.trainable(n))
        return net


def _mixed_bn(prefix):
    """Every odd-numbered conv_bn_relu (counted from 0 in graph order, the heads not counted) in eval mode; the train-mode ones of
    pre_det2 average cumulatively from two tracked batches (factor 1/3), those of pre_det3 use momentum 0.03 and eps 1e-3."""
    training = cbr_prefixes().index(prefix) % 2 == 0
    if training and prefix.startswith("pre_det2."):
        return True, None, EPS, 2
    if training and prefix.startswith("pre_det3."):
        return True, 0.03, 1e-3, 0
    return training, MOMENTUM, EPS, 0


def _conv1_of_a_block(name):
    return name.endswith(".conv1.conv.weight") and name.rsplit(".", 3)[0] in res_blocks()


ALL_TRAIN = State("all_train", lambda n: True)
ALL_EVAL = State("all_eval", lambda n: True, lambda p: (False, MOMENTUM, EPS, 0))
STATES = {s.name: s for s in (
    State("bn_frozen", lambda n: not _is_bn_param(n), lambda p: (False, MOMENTUM, EPS, 0)),
    State("backbone_eval_frozen", lambda n: not n.startswith("feature."), lambda p: (not p.startswith("feature."), MOMENTUM, EPS, 0),
          modes=lambda net: net.feature.eval()),
    State("mixed_bn", lambda n: True, _mixed_bn),
    State("bn_only", _is_bn_param),
    State("island", lambda n: n.startswith("feature.mlist.2.")),
    State("pre_det3_only", lambda n: n.startswith("pre_det3.")),
    State("block_halves", lambda n: not _conv1_of_a_block(n)),
)}


def pick_target(logit_sets, size, num_class, batch, rows=8, seed=77):
    """Target rows by the margins rule of tests/test_gpu_train.py's pick_target (every decision clears the 1e-4 margins, at least one
    ground truth), held on each of `logit_sets` (the three heads' float64 logits of one or more restatements) at once."""
    for attempt in range(100):
        tg = R.random_rows(seed * 1000 + attempt, batch, rows, num_class, (0.03, 0.8), n_valid_lo=3)
        res = [T.head_losses(logits, tg, size, num_class) for logits in logit_sets]
        if all(R.margins_ok(r["margins"]) for rs in res for r in rs) and all(sum(r["nGT"] for r in rs) > 0 for rs in res):
            return tg
    raise AssertionError("no target draw clears the margins")


# ---------------------------------------------------------------- the need rule, from backprop.py's docstring
def op_prefix(op):
    """The module name of one op of backprop.graph(net), read off the buffer it writes."""
    out = op.out
    if out.startswith("f"):
        pos = out[1:].rstrip("a")
        if out.endswith("a"):
            return "feature.mlist.%s.conv1" % pos
        return "feature.mlist.%s%s" % (pos, ".conv2" if op.res is not None else "")
    if out in ("up1", "up2"):
        return out + ".conv"
    group, i = out.split(".")
    return "%s.mlist.%s" % (group, "6" if i == "logits" else i)


def op_param_names(op):
    """(conv weight, the op's other parameters) in state_dict names."""
    p = op_prefix(op)
    if op.head:
        return p + ".weight", [p + ".bias"]
    return p + ".conv.weight", [p + ".bn.weight", p + ".bn.bias"]


def expected_walk(state, ops):
    """Per op index: None when the reverse walk must not visit the op, else the set of WALK_KEYS its trace must hold.

    The rule ("Backward stops at the first layer whose inputs need no gradient"; the input image needs none here): a buffer is needed
    when a parameter of the op that writes it is trainable or one of that op's inputs is needed; an op is walked when its output is
    needed; it computes dw when its conv weight is trainable, runs its dgrad when one of its inputs is needed (writing straight into
    the input's gradient, or through the upsample/concat split into whichever of the two inputs is needed), and hands dy to its
    residual input when that is needed."""
    needed = {"x": False}
    for op in ops:
        w, others = op_param_names(op)
        inputs = [b for b in (op.src, op.src2, op.res) if b is not None]
        needed[op.out] = any(state.trainable(n) for n in [w] + others) or any(needed[b] for b in inputs)
    out = {}
    for i, op in enumerate(ops):
        if not needed[op.out]:
            out[i] = None
            continue
        keys = set()
        if state.trainable(op_param_names(op)[0]):
            keys.add("dw")
        if op.res is not None and needed[op.res]:
            keys.add("res_after")
        if op.src2 is None:
            if needed[op.src]:
                keys.add("dx_after")
        elif needed[op.src] or needed[op.src2]:
            keys.add("dcat")
            if needed[op.src2]:
                keys.add("dlow_after")
            if needed[op.src]:
                keys.add("dtail_after")
        out[i] = keys
    return out
