"""backprop.frozen_prefix_ops: how many leading ops of a YoloNet a training step may hand to the inference engine
(net.frozen_prefix).  CPU only; the answers are written by hand from the graph: 52 backbone ops (feature.mlist.0, then per stage a
stride-2 conv and its residual blocks' conv1 / conv2), pre_det1 (7), up1.conv, pre_det2 (7), up2.conv, pre_det3 (7)."""
import copy
import functools

import pytest

from tests import train_states as S
from tests.frozen_prefix_check import frozen_through, CUTS, HANDED
from yolo_v3_amd import arch

C = 3
EVERY = dict(S.STATES, all_train=S.ALL_TRAIN, all_eval=S.ALL_EVAL)
# every state of tests/train_states.py: the train-mode ones have a train-mode BatchNorm in op 0, bn_frozen and all_eval a trainable
# weight there; only the eval-mode frozen backbone has a prefix, the backbone's 52 ops
BY_STATE = {"bn_frozen": 0, "backbone_eval_frozen": 52, "mixed_bn": 0, "bn_only": 0, "island": 0, "pre_det3_only": 0,
            "block_halves": 0, "all_train": 0, "all_eval": 0}


@functools.lru_cache(maxsize=None)
def cpu_net():
    from yolo_v3_amd import YoloNet
    return YoloNet((96, 96), numClass=C)


def test_the_graph_runs_the_convolutions_in_conv_specs_order():
    """The prefix engine packs arch.conv_specs(...)[:n] for the first n ops of the graph: the two orders are one, name by name."""
    from yolo_v3_amd import backprop
    ops = backprop.graph(cpu_net())
    specs = arch.conv_specs(C)
    assert len(ops) == len(specs) == 75
    mods = dict(cpu_net().named_modules())
    for op, sp in zip(ops, specs):
        assert S.op_prefix(op) == sp.name and mods[sp.name] is op.module, (op.out, sp.name)
        assert op.head == (not sp.bn) and (op.conv.in_channels, op.conv.out_channels) == (sp.cin, sp.cout)


def test_the_states_are_all_there():
    assert sorted(BY_STATE) == sorted(EVERY) and len(S.STATES) == 7


@pytest.mark.parametrize("name", sorted(BY_STATE))
def test_prefix_of_each_state(name):
    from yolo_v3_amd import backprop
    net = EVERY[name].apply(copy.deepcopy(cpu_net()))
    assert backprop.frozen_prefix_ops(net) == BY_STATE[name]
    assert backprop.frozen_prefix_ops(net, input_grad=True) == 0


def test_everything_but_pre_det3_frozen_in_eval_mode():
    from yolo_v3_amd import backprop
    net = copy.deepcopy(cpu_net()).eval()
    for n, p in net.named_parameters():
        p.requires_grad_(n.startswith("pre_det3."))
    assert backprop.frozen_prefix_ops(net) == 68                 # 52 + 7 + 1 + 7 + 1: two frozen heads are inside the run
    assert backprop.frozen_prefix_ops(net, input_grad=True) == 0
    net.pre_det1.mlist[6].bias.requires_grad_(True)              # the first head's bias alone ends the run in front of it
    assert backprop.frozen_prefix_ops(net) == 58


def test_everything_frozen_in_eval_mode():
    from yolo_v3_amd import backprop
    net = copy.deepcopy(cpu_net()).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    assert backprop.frozen_prefix_ops(net) == 75
    net.train()                                                  # the reference's freeze_backbone=True alone: BatchNorm still trains
    assert backprop.frozen_prefix_ops(net) == 0


def test_requires_grad_false_alone_is_no_prefix():
    """The reference's get_optimizer(freeze_backbone=True) only clears requires_grad: the backbone's BatchNorms stay in train mode."""
    from yolo_v3_amd import backprop
    net = copy.deepcopy(cpu_net()).train()
    for p in net.feature.parameters():
        p.requires_grad_(False)
    assert backprop.frozen_prefix_ops(net) == 0
    net.feature.eval()
    assert backprop.frozen_prefix_ops(net) == 52


def test_a_cut_inside_a_residual_block():
    from yolo_v3_amd import backprop
    net = frozen_through("feature.mlist.5.conv1").apply(copy.deepcopy(cpu_net()))
    assert backprop.frozen_prefix_ops(net) == 8                  # mlist.0, .1, .2 (2), .3, .4 (2), .5.conv1
    ops = backprop.graph(net)
    assert (ops[8].src, ops[8].res) == ("f5a", "f4") and ops[7].out == "f5a" and ops[6].out == "f4"
    assert backprop.frozen_prefix_ops(net, input_grad=True) == 0


@pytest.mark.parametrize("last,n", [("feature.mlist.2.conv1", 0), ("feature.mlist.2.conv2", 4), ("feature.mlist.3", 5)])
def test_a_run_shorter_than_the_fused_front_is_no_prefix(last, n):
    from yolo_v3_amd import backprop
    net = frozen_through(last).apply(copy.deepcopy(cpu_net()))
    assert backprop.frozen_prefix_ops(net) == n                  # 3 ops: inside the fused launches, nothing to hand over


def test_a_train_mode_batchnorm_ends_the_run():
    from yolo_v3_amd import backprop
    net = S.STATES["backbone_eval_frozen"].apply(copy.deepcopy(cpu_net()))
    net.feature.mlist[7].conv2.bn.train()
    names = [sp.name for sp in arch.conv_specs(C)]
    assert backprop.frozen_prefix_ops(net) == names.index("feature.mlist.7.conv2")


def test_the_switch_is_off_by_default_and_not_part_of_the_copies():
    import pickle
    net = cpu_net()
    assert net.frozen_prefix is False and net._prefix_engines == {}
    twin = copy.deepcopy(net)
    twin.frozen_prefix = True
    twin._prefix_engines[(0, 52)] = object()
    assert copy.deepcopy(twin)._prefix_engines == {} and copy.deepcopy(twin).frozen_prefix is True
    assert pickle.loads(pickle.dumps(net))._prefix_engines == {}
    twin.repack()
    assert twin._prefix_engines == {}
    twin._prefix_engines[(0, 52)] = object()
    twin.load_state_dict(net.state_dict())
    assert twin._prefix_engines == {}


def test_an_engine_covers_the_front_at_least():
    from yolo_v3_amd import engine, Yv3Error, F32
    net = cpu_net()
    for n in (0, 3, 76):
        with pytest.raises(Yv3Error):
            engine.Engine(net, F32, n)
    eng = engine.Engine(net, F32, 8)
    with pytest.raises(Yv3Error, match="no detections"):            # (before anything touches the GPU)
        eng.forward(None)
    assert [sp.name for sp in eng.specs] == [sp.name for sp in arch.conv_specs(C)[:8]] and len(eng.all_specs) == 75
    assert len(engine.Engine(net, F32).specs) == 75
    # its signature is built from those layers' tensors only: 5 per conv_bn_relu (weight, gamma, beta, running mean / variance)
    assert len(eng._param_tensors()) == 5 * 8
    mods = dict(net.named_modules())
    want = [t for sp in arch.conv_specs(C)[:8] for m in [mods[sp.name]]
            for t in (m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var)]
    assert all(a is b for a, b in zip(eng._param_tensors(), want))
    assert len(engine.Engine(net, F32, 59)._param_tensors()) == 5 * 58 + 2          # with pre_det1's head: weight and bias


@pytest.mark.parametrize("n", sorted(CUTS))
def test_the_cuts_of_the_gpu_tests(n):
    """The three states tests/test_gpu_frozen_prefix.py runs give the prefix they are named by, and the buffers written down as handed
    over are the prefix's outputs that an op from n on reads."""
    from yolo_v3_amd import backprop
    net = CUTS[n].apply(copy.deepcopy(cpu_net()))
    assert backprop.frozen_prefix_ops(net) == n
    ops = backprop.graph(net)
    wrote = {op.out for op in ops[:n]}
    src = {b for op in ops[n:] for b in (op.src, op.src2) if b in wrote}
    res = {op.res for op in ops[n:] if op.res in wrote}
    heads = {op.out for op in ops[:n] if op.head}
    assert (src, res, heads) == HANDED[n]
    walk = S.expected_walk(CUTS[n], ops)
    assert all(walk[i] is None for i in range(n)) and all(walk[i] is not None and "dw" in walk[i] for i in range(n, 75))
