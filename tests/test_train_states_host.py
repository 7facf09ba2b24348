"""The fine-tuning states of tests/train_states.py and the `state=` keyword of the float64 restatements (tests/train_ref.py,
train_ref_bf16.py, train_ref_bf16_act.py).  CPU only.

The restatements with a state are checked three ways: the two uniform states reproduce the `train=` flag bit for bit, freezing
parameters changes no bit of the gradients that are left, and BatchNorms that differ from their neighbours behave as a plain
nn.BatchNorm2d with the same settings does on the same float64 input.  expected_walk is checked against answers written by hand from
the graph (Darknet-53's 52 backbone ops, then pre_det1, up1, pre_det2, up2, pre_det3)."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

from tests import test_train_host as H
from tests import train_kernel_ref as K
from tests import train_ref as T
from tests import train_ref_bf16 as TB
from tests import train_ref_bf16_act as TA
from tests import train_states as S

C = H.CASE["C"]
MODS = {"f32": T, "bf16": TB, "bf16_act": TA}
EVERY = dict(S.STATES, all_train=S.ALL_TRAIN, all_eval=S.ALL_EVAL)


@functools.lru_cache(maxsize=None)
def cpu_net():
    from yolo_v3_amd import YoloNet
    return YoloNet((96, 96), numClass=C)


@functools.lru_cache(maxsize=None)
def inputs():
    """(state_dict, x, target) of the small training case: 96x96, B=2, C=3, eight target rows clearing the margins."""
    from yolo_v3_amd import synth
    sd = H.state_dict()
    x = torch.from_numpy(synth.images(2, 96, 31))
    return sd, x, S.pick_target([T.forward(sd, x)[0]], 96, C, 2)


@functools.lru_cache(maxsize=None)
def flag_run(mod, train):
    sd, x, tg = inputs()
    return MODS[mod].run(sd, x, tg, C, train=train)


def same_step(a, b):
    assert a["loss"] == b["loss"] and a["stats"] == b["stats"]
    assert list(a["grads"]) == list(b["grads"]) and list(a["running"]) == list(b["running"])
    for k, g in a["grads"].items():
        assert g is not None and torch.equal(g, b["grads"][k]), k
    for k, (m, v) in a["running"].items():
        assert torch.equal(m, b["running"][k][0]) and torch.equal(v, b["running"][k][1]), k


# ---------------------------------------------------------------- the states say the same thing three ways
def test_the_names_are_the_graphs():
    from yolo_v3_amd import backprop
    net = cpu_net()
    ops = backprop.graph(net)
    keys = K.op_params(net, ops)
    assert [kbn[:-3] for _, _, kbn in keys if kbn] == S.cbr_prefixes() and len(S.cbr_prefixes()) == 72
    for op, (kw, kb, kbn) in zip(ops, keys):
        assert S.op_param_names(op) == (kw, [kb] if op.head else [kbn + ".weight", kbn + ".bias"]), op.out
    assert "feature.mlist.2" in S.res_blocks() and "feature.mlist.1" not in S.res_blocks() and len(S.res_blocks()) == 23
    by_op = [n for op in ops for n in [S.op_param_names(op)[0]] + S.op_param_names(op)[1]]
    assert sorted(T.param_names(net.state_dict())) == sorted(by_op)


@pytest.mark.parametrize("name", sorted(EVERY))
def test_apply_agrees_with_trainable_and_bn(name):
    state = EVERY[name]
    net = state.apply(copy.deepcopy(cpu_net()))
    named = dict(net.named_parameters())
    assert sorted(named) == sorted(T.param_names(net.state_dict()))
    for n, p in named.items():
        assert p.requires_grad == state.trainable(n), n
    mods = dict(net.named_modules())
    bns = {n[:-3]: m for n, m in mods.items() if isinstance(m, nn.BatchNorm2d)}
    assert sorted(bns) == sorted(S.cbr_prefixes())
    for prefix, m in bns.items():
        assert (m.training, m.momentum, m.eps, int(m.num_batches_tracked)) == state.bn(prefix), prefix
        assert state.bn(prefix + ".bn") == state.bn(prefix)
    modes_only = state.apply_modes(copy.deepcopy(cpu_net()))
    assert all(p.requires_grad for p in modes_only.parameters())
    assert all(mods[n].training == m.training for n, m in modes_only.named_modules() if isinstance(m, nn.BatchNorm2d))


def test_the_states_are_the_issues():
    """The table of the states, spelled out on names."""
    s = S.STATES
    assert sorted(s) == ["backbone_eval_frozen", "block_halves", "bn_frozen", "bn_only", "island", "mixed_bn", "pre_det3_only"]
    names = T.param_names(cpu_net().state_dict())
    count = {k: sum(v.trainable(n) for n in names) for k, v in s.items()}
    # 75 conv weights, 72 BN pairs, 3 head biases; the backbone holds 52 convs; 23 residual blocks
    assert count == dict(bn_frozen=75 + 3, backbone_eval_frozen=222 - 3 * 52, mixed_bn=222, bn_only=144, island=6,
                         pre_det3_only=6 * 3 + 2, block_halves=222 - 23)
    assert [n for n in names if s["island"].trainable(n)] == ["feature.mlist.2.conv%d.%s" % (i, t) for i in (1, 2)
                                                               for t in ("conv.weight", "bn.weight", "bn.bias")]
    halves = s["block_halves"]
    assert not halves.trainable("feature.mlist.2.conv1.conv.weight") and halves.trainable("feature.mlist.2.conv1.bn.weight")
    assert halves.trainable("feature.mlist.2.conv2.conv.weight") and halves.trainable("feature.mlist.1.conv.weight")
    assert s["bn_frozen"].uniform_bn() is False
    assert s["backbone_eval_frozen"].uniform_bn() is None and s["mixed_bn"].uniform_bn() is None
    assert all(s[k].uniform_bn() is True for k in ("bn_only", "island", "pre_det3_only", "block_halves"))
    m, order = s["mixed_bn"], S.cbr_prefixes()
    assert [m.bn(p)[0] for p in order] == [i % 2 == 0 for i in range(72)]
    assert order.index("pre_det2.mlist.1") == 60 and m.bn("pre_det2.mlist.1") == (True, None, 1e-5, 2)
    assert m.factor("pre_det2.mlist.1") == 1.0 / 3 and m.factor("pre_det3.mlist.0") == 0.03
    assert m.bn("pre_det2.mlist.0") == (False, 0.1, 1e-5, 0) and m.bn("pre_det3.mlist.0") == (True, 0.03, 1e-3, 0)
    assert m.bn("pre_det3.mlist.1") == (False, 0.1, 1e-5, 0) and m.bn("feature.mlist.0") == (True, 0.1, 1e-5, 0)
    assert s["backbone_eval_frozen"].bn("feature.mlist.1")[0] is False and s["backbone_eval_frozen"].bn("up1.conv")[0] is True


# ---------------------------------------------------------------- the restatements under a state
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("mod", sorted(MODS))
def test_a_uniform_state_is_the_train_flag_bitwise(mod, train):
    sd, x, tg = inputs()
    same_step(flag_run(mod, train), MODS[mod].run(sd, x, tg, C, state=S.ALL_TRAIN if train else S.ALL_EVAL))


@pytest.mark.parametrize("name", [k for k, v in sorted(S.STATES.items()) if v.uniform_bn() is not None])
def test_freezing_changes_no_bit_of_the_restatement(name):
    state = S.STATES[name]
    sd, x, tg = inputs()
    full = flag_run("f32", state.uniform_bn())
    got = T.run(sd, x, tg, C, state=state)
    assert got["loss"] == full["loss"] and got["stats"] == full["stats"]
    assert any(g is None for g in got["grads"].values()) and any(g is not None for g in got["grads"].values())
    for k, g in got["grads"].items():
        if state.trainable(k):
            assert g is not None and torch.equal(g, full["grads"][k]), k
        else:
            assert g is None, k
    for k, (m, v) in full["running"].items():
        assert torch.equal(m, got["running"][k][0]) and torch.equal(v, got["running"][k][1]), k


def test_mixed_batchnorms_speak_torchs_semantics(monkeypatch):
    state = S.STATES["mixed_bn"]
    sd, x, tg = inputs()
    seen, real = [], torch.nn.functional.batch_norm

    def recording(z, rm, rv, weight, bias, **kw):
        seen.append(dict(z=z.detach().clone(), rm=rm.clone(), rv=rv.clone(), w=weight.detach().clone(), b=bias.detach().clone()))
        seen[-1]["y"] = real(z, rm, rv, weight, bias, **kw)
        return seen[-1]["y"]

    with monkeypatch.context() as m:
        m.setattr(T.F, "batch_norm", recording)
        out = T.run(sd, x, tg, C, state=state)
    order = S.cbr_prefixes()
    assert len(seen) == 72 and list(out["running"]) == order         # (the forward calls the BatchNorms in graph order)
    cumulative = [p for p in order if state.bn(p)[1] is None]
    assert cumulative == ["pre_det2.mlist.1", "pre_det2.mlist.3", "pre_det2.mlist.5"]
    for p, rec in zip(order, seen):
        training, momentum, eps, nbt = state.bn(p)
        old_m, old_v = sd[p + ".bn.running_mean"].double(), sd[p + ".bn.running_var"].double()
        new_m, new_v = out["running"][p]
        assert torch.equal(rec["rm"], old_m) and torch.equal(rec["rv"], old_v)
        if not training:
            assert torch.equal(new_m, old_m) and torch.equal(new_v, old_v), p
            continue
        assert not torch.equal(new_m, old_m) and not torch.equal(new_v, old_v), p
        zr = K.rows(rec["z"])
        mean, var, _ = K.bn_batch_stats(zr, eps)
        if p in cumulative:                      # (2/3) old + (1/3) batch, the variance unbiased; float64 leaves a few ulp
            unb = var * (zr.shape[0] / (zr.shape[0] - 1.0))
            assert T.rel_l2(new_m, old_m * 2 / 3 + mean / 3) <= 1e-14 and T.rel_l2(new_v, old_v * 2 / 3 + unb / 3) <= 1e-14, p
        want_m, want_v = K.bn_running(mean, var, zr.shape[0], old_m, old_v, state.factor(p))
        assert T.rel_l2(new_m, want_m) <= 1e-14 and T.rel_l2(new_v, want_v) <= 1e-14, p
        # a plain nn.BatchNorm2d with the state's settings on the same z: bitwise the restatement's layer
        bn = nn.BatchNorm2d(zr.shape[1], eps=eps, momentum=momentum).double()
        with torch.no_grad():
            bn.weight.copy_(rec["w"])
            bn.bias.copy_(rec["b"])
            bn.running_mean.copy_(old_m)
            bn.running_var.copy_(old_v)
            bn.num_batches_tracked.fill_(nbt)
            y = bn.train()(rec["z"])
        assert torch.equal(y, rec["y"].detach()), p
        assert torch.equal(bn.running_mean, new_m) and torch.equal(bn.running_var, new_v), p
        assert int(bn.num_batches_tracked) == nbt + 1


# ---------------------------------------------------------------- expected_walk against answers written by hand
def graph_ops():
    from yolo_v3_amd import backprop
    ops = backprop.graph(cpu_net())
    assert len(ops) == 75
    return ops, [op.out for op in ops]


def test_walk_all_trainable_is_what_check_step_assumes():
    ops, outs = graph_ops()
    walk = S.expected_walk(S.ALL_TRAIN, ops)
    assert sorted(walk) == list(range(75))
    for i, op in enumerate(ops):
        if op.src == "x":
            want = {"dw"}
        elif op.cin_up:
            want = {"dw", "dcat", "dlow_after", "dtail_after"}
        elif op.res is not None:
            want = {"dw", "dx_after", "res_after"}
        else:
            want = {"dw", "dx_after"}
        assert walk[i] == want, op.out
    assert sum(op.res is not None for op in ops) == 23 and [op.out for op in ops if op.cin_up] == ["pre_det2.0", "pre_det3.0"]
    assert S.expected_walk(S.STATES["mixed_bn"], ops) == walk and S.expected_walk(S.STATES["bn_frozen"], ops) == walk
    halves = S.expected_walk(S.STATES["block_halves"], ops)
    assert all(halves[i] == (walk[i] - {"dw"} if op.out.endswith("a") else walk[i]) for i, op in enumerate(ops))


def test_walk_island():
    ops, outs = graph_ops()
    walk = S.expected_walk(S.STATES["island"], ops)
    c1, c2 = outs.index("f2a"), outs.index("f2")
    assert (c1, c2) == (2, 3) and ops[c2].res == "f1" and ops[c1].src == "f1"
    assert [i for i in range(75) if walk[i] is None] == [0, 1]
    assert [i for i in range(75) if walk[i] and "dw" in walk[i]] == [c1, c2]
    assert walk[c1] == {"dw"} and walk[c2] == {"dw", "dx_after"}           # nothing below conv1 is needed: no dgrad, no residual hand-over
    full = S.expected_walk(S.ALL_TRAIN, ops)
    assert all(walk[i] == full[i] - {"dw"} for i in range(4, 75))           # downstream: every dgrad and hand-over, no wgrad


def test_walk_pre_det3_only():
    ops, outs = graph_ops()
    walk = S.expected_walk(S.STATES["pre_det3_only"], ops)
    walked = [i for i in range(75) if walk[i] is not None]
    assert [outs[i] for i in walked] == ["pre_det3.%d" % i for i in range(6)] + ["pre_det3.logits"] and walked == list(range(68, 75))
    assert walk[68] == {"dw"}                                               # neither the route tail nor up2 is needed: no dcat
    assert all(walk[i] == {"dw", "dx_after"} for i in range(69, 75))


def test_walk_bn_only():
    ops, outs = graph_ops()
    walk = S.expected_walk(S.STATES["bn_only"], ops)
    full = S.expected_walk(S.ALL_TRAIN, ops)
    assert walk[0] == set() and all(walk[i] == full[i] - {"dw"} and walk[i] & {"dx_after", "dcat"} for i in range(1, 75))


def test_walk_frozen_backbone():
    ops, outs = graph_ops()
    walk = S.expected_walk(S.STATES["backbone_eval_frozen"], ops)
    assert [i for i in range(75) if walk[i] is None] == list(range(52))
    assert walk[outs.index("pre_det1.0")] == {"dw"}                         # the backbone's last buffer is not needed
    assert walk[outs.index("pre_det2.0")] == {"dw", "dcat", "dlow_after"}   # up1 is needed, the route tail is not
    assert walk[outs.index("pre_det3.0")] == {"dw", "dcat", "dlow_after"}
    rest = set(range(52, 75)) - {outs.index("pre_det%d.0" % k) for k in (1, 2, 3)}
    assert all(walk[i] == {"dw", "dx_after"} for i in rest)
