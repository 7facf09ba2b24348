"""One training step under the module states a fine-tuning run uses (tests/train_states.py): BatchNorm frozen in eval mode under
trainable convolutions, an eval-mode backbone under train-mode heads, alternating BatchNorm modes with per-module momentum / eps,
BN-only tuning, one trainable block, one trainable branch, every block's first weight frozen.  All at 96x96, B=2, C=3.

Three kinds of check, each where it is the sharpest:

(a) the states whose BatchNorms are not uniform, op by op against float64 on the GPU's own inputs (test_gpu_train_local.check_step
    with the state: each op's own mode, momentum and eps, and the walked ops and their trace keys exactly expected_walk's) in F32 and
    BF16; in BF16_ACT as whole steps against tests/train_ref_bf16_act.py under the same state.  The other states run the same walk
    check without the float64 part: their arithmetic is (b)'s.
(b) every state, in the three math modes, bitwise against the all-trainable step under the same BatchNorm modes: the kernels sum in a
    fixed order and a needed buffer receives all its contributions in that order, so freezing parameters changes no bit of what is
    still computed.
(c) BF16_ACT: after the forward the run holds exactly the bf16 buffers a wgrad of the walk will read, and z of exactly the walked ops.
(d) the logits path (net.logits, the YOLO layers on the logits, autograd) under a state: bitwise the loss path's gradients.

The bars are those of the checkers used (CONV_BAR, BN_BAR, KINK_SHARE; 16x the fp32 CPU run of the same state); none is new."""
import copy
import functools

import pytest
import torch

from tests import test_gpu_train_bf16 as GB
from tests import test_gpu_train_bf16_act_step as A
from tests import test_gpu_train_local as L
from tests import test_train_host as H
from tests import train_ref as T
from tests import train_ref_bf16 as TB
from tests import train_ref_bf16_act as TA
from tests import train_states as S
from yolo_v3_amd import backprop, F32, BF16, BF16_ACT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HW, C, B = (96, 96), 3, 2
MATHS = {"f32": F32, "bf16": BF16, "bf16_act": BF16_ACT}
MIXED = ["bn_frozen", "backbone_eval_frozen", "mixed_bn"]            # the states whose BatchNorms are not all in train mode
UNIFORM = [n for n in S.STATES if n not in MIXED]


@functools.lru_cache(maxsize=None)
def inputs():
    return H.state_dict(), L.images(B, HW, 31)


_targets = {}


def case(name):
    """(state_dict, x, target): the target clears the margins on the float64 logits of all three restatements under the state
    (computed once per set of BatchNorm settings and left unchanged)."""
    state = S.STATES[name]
    sd, x = inputs()
    sig = tuple(state.bn(p) for p in S.cbr_prefixes())
    if sig not in _targets:
        _targets[sig] = S.pick_target([m.forward(sd, x, state=state)[0] for m in (T, TB, TA)], HW[0], C, B)
    return sd, x, _targets[sig]


@functools.lru_cache(maxsize=None)
def act_refs(name):
    """The float64 BF16_ACT step under the state and the same step in fp32 on the CPU."""
    sd, x, tg = case(name)
    return (TA.run(sd, x, tg, C, state=S.STATES[name]), TA.run(sd, x, tg, C, state=S.STATES[name], dtype=torch.float32))


def make_net(name, math, freeze=True):
    net = L.make_net(HW, C, math)
    return S.STATES[name].apply(net) if freeze else S.STATES[name].apply_modes(net)


def tracked(net):
    return {p: int(dict(net.named_modules())[p].bn.num_batches_tracked) for p in S.cbr_prefixes()}


def assert_tracked_moved(state, before, net):
    after = tracked(net)
    for p in S.cbr_prefixes():
        assert before[p] == state.bn(p)[3] and after[p] == before[p] + int(state.bn(p)[0]), p


def assert_grads_where_trainable(state, net):
    for n, p in net.named_parameters():
        assert (p.grad is None) == (not state.trainable(n)), n


def assert_same_step(state, a, la, b, lb):
    """Loss, stats, every state_dict entry and the gradients of the state's trainable parameters: bitwise."""
    assert torch.equal(la.detach(), lb.detach()) and a.stats == b.stats
    for (k, v), (k2, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k
    gb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        if state.trainable(n):
            assert p.grad is not None and gb[n].grad is not None and torch.equal(p.grad, gb[n].grad), n


def walked_param_ids(net, run, walk):
    named = dict(net.named_parameters())
    out = set()
    for i, op in enumerate(run.ops):
        if walk[i] is not None:
            w, others = S.op_param_names(op)
            out.update(id(named[n]) for n in others + ([w] if "dw" in walk[i] else []))
    return out


# ---------------------------------------------------------------- (a) op by op against float64 on the GPU's own inputs
def traced_case(name, math):
    state = S.STATES[name]
    _, x, tg = case(name)
    net = make_net(name, math)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    nbt = tracked(net)
    twin = copy.deepcopy(net)
    run, loss, pg = L.traced_step(net, x, tg)
    assert_tracked_moved(state, nbt, net)
    l2 = GB.gpu_step(twin, x, tg)                       # a plain step (trace off): bitwise the traced one
    assert float(l2.detach()) == float(loss)
    assert_grads_where_trainable(state, twin)
    for (n, p), (_, q) in zip(net.named_parameters(), twin.named_parameters()):
        assert q.grad is None or torch.equal(q.grad, pg[id(p)].view_as(q)), n
    for (k, v), (_, v2) in zip(net.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(v, v2), k
    return state, net, sd, run, pg


@pytest.mark.parametrize("math", ["f32", "bf16"])
@pytest.mark.parametrize("name", MIXED)
def test_every_op_against_float64_under_a_state(name, math):
    state, net, sd, run, pg = traced_case(name, MATHS[math])
    L.check_step(net, sd, run, pg, None, "%s %s 96x96 B=2" % (name, math.upper()), state=state)


@pytest.mark.parametrize("name", UNIFORM)
def test_the_walk_visits_what_the_state_needs(name):
    """The states (a) leaves to (b): the traced F32 walk visits exactly expected_walk's ops, each trace holds exactly its keys, the
    walk returns exactly the walked ops' gradients."""
    state, net, sd, run, pg = traced_case(name, F32)
    walk = S.expected_walk(state, run.ops)
    assert sorted(run.trace) == [i for i in range(75) if walk[i] is not None]
    for i, t in run.trace.items():
        assert set(t) & set(S.WALK_KEYS) == walk[i], (run.ops[i].out, sorted(t), sorted(walk[i]))
    assert set(pg) == walked_param_ids(net, run, walk)


@pytest.mark.parametrize("name", MIXED)
def test_bf16_act_step_matches_float64_under_a_state(name):
    state = S.STATES[name]
    _, x, tg = case(name)
    ref, ref32 = act_refs(name)
    net = make_net(name, BF16_ACT)
    nbt = tracked(net)
    loss = GB.gpu_step(net, x, tg)
    assert loss.requires_grad
    print("BF16_ACT %s:" % name, end=" ")
    A.check_against_ref(net, loss, ref, ref32, lambda prefix: state.bn(prefix)[0])       # (eval-mode statistics: bitwise unchanged)
    assert_grads_where_trainable(state, net)
    assert_tracked_moved(state, nbt, net)


# ---------------------------------------------------------------- (b) bitwise against the all-trainable step
@pytest.mark.parametrize("math", sorted(MATHS))
@pytest.mark.parametrize("name", sorted(S.STATES))
def test_freezing_changes_no_bit(name, math):
    state = S.STATES[name]
    _, x, tg = case(name)
    frozen, full = make_net(name, MATHS[math]), make_net(name, MATHS[math], freeze=False)
    assert all(p.requires_grad for p in full.parameters())
    nbt = tracked(frozen)
    lf, la = GB.gpu_step(frozen, x, tg), GB.gpu_step(full, x, tg)
    assert_same_step(state, frozen, lf, full, la)
    assert_grads_where_trainable(state, frozen)
    assert all(p.grad is not None for p in full.parameters())
    assert_tracked_moved(state, nbt, frozen)
    assert_tracked_moved(state, nbt, full)


# ---------------------------------------------------------------- (c) BF16_ACT: what the run holds after the forward
@pytest.mark.parametrize("name", sorted(S.STATES))
def test_bf16_act_holds_what_the_walk_reads(name):
    """A bf16 buffer lives until its last reader, a later op or a wgrad of the walk: after the forward exactly the inputs of the ops
    that will run a wgrad are left (the image's bf16 copy and the last layer's input among them only then), and z of exactly the
    walked conv_bn_relu ops.  A buffer freed too early would show as a KeyError in the walk, not as a GPU fault."""
    state = S.STATES[name]
    _, x, tg = case(name)
    net = make_net(name, BF16_ACT)
    run = backprop._Run(net, x.to(DEV).float().contiguous(), torch.as_tensor(tg), BF16_ACT)
    with torch.no_grad():
        backprop.forward(run, want_grad=True)
    torch.cuda.synchronize()
    walk = S.expected_walk(state, run.ops)
    readers = [op for i, op in enumerate(run.ops) if walk[i] is not None and "dw" in walk[i]]
    assert sorted(run.bufs_b) == sorted({b for op in readers for b in (op.src, op.src2) if b is not None})
    assert sorted(run.bufs) == sorted(["x"] + [op.out for op in run.ops if op.head])
    for i, op in enumerate(run.ops):
        if not op.head:
            assert (run.saved[i]["z"] is None) == (walk[i] is None), op.out
    if name == "bn_only":
        assert not run.bufs_b                           # no activation survives but z
    with torch.no_grad():
        pg = backprop.backward(run, torch.ones((), device=DEV))
    torch.cuda.synchronize()
    assert set(pg) == walked_param_ids(net, run, walk)
    assert all(torch.isfinite(g).all() for g in pg.values())


# ---------------------------------------------------------------- (d) the logits path under a state
def logits_step(net, x, tg, heads=(0, 1, 2)):
    lg = net.logits(x.to(DEV))
    layers = (net.yolo1, net.yolo2, net.yolo3)
    loss = sum(layers[k](lg[k], net.img_dim, torch.as_tensor(tg))[0] for k in heads)
    loss.backward()
    torch.cuda.synchronize()
    return loss


@pytest.mark.parametrize("math", ["f32", "bf16_act"])
def test_yolo_layers_on_logits_are_the_training_step_on_an_island(math):
    state = S.STATES["island"]
    _, x, tg = case("island")
    a, b = make_net("island", MATHS[math]), make_net("island", MATHS[math])
    la, lb = logits_step(a, x, tg), GB.gpu_step(b, x, tg)
    assert float(la.detach()) == float(lb.detach())
    assert_grads_where_trainable(state, a)
    assert_grads_where_trainable(state, b)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert p.grad is None or torch.equal(p.grad, q.grad), n
    for (k, v), (_, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(v, v2), k


@pytest.mark.parametrize("math", ["f32", "bf16_act"])
def test_pre_det3_sees_only_its_own_head(math):
    state = S.STATES["pre_det3_only"]
    _, x, tg = case("pre_det3_only")
    one, three = make_net("pre_det3_only", MATHS[math]), make_net("pre_det3_only", MATHS[math])
    logits_step(one, x, tg, heads=(2,))
    GB.gpu_step(three, x, tg)
    assert_grads_where_trainable(state, one)
    assert_grads_where_trainable(state, three)
    for (n, p), (_, q) in zip(one.named_parameters(), three.named_parameters()):
        assert p.grad is None or (n.startswith("pre_det3.") and torch.equal(p.grad, q.grad)), n
