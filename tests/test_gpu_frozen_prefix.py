"""net.frozen_prefix: the frozen eval-mode prefix of a training step on the inference engine (yolo_v3_amd/backprop.py _prefix,
engine.Engine with n_conv).  96x96, B=2, C=3, one step each, in F32, BF16 and BF16_ACT, for the three cuts of
tests/frozen_prefix_check.py: n = 52 (the eval-mode frozen backbone), 68 (everything but pre_det3 frozen, the net in .eval(): two
frozen heads and both upsample convs inside the prefix) and 8 (a cut inside a residual block: a residual read from the prefix).

* The hand-over is bitwise the inference engine: every buffer the prefix hands to the training kernels equals the same-named
  layer_out / logits of the full 75-layer logits plan of that mode on the same net and x -- the same launches, no tolerance -- in
  the form its reader expects, as a copy that shares no memory with the plan.
* The training kernels are unchanged: ops >= n op by op against float64 on the GPU's own inputs (frozen_prefix_check.check_from, the
  existing bars), the walked ops and trace keys exactly expected_walk's.
* State is untouched: no run.saved entry below n, grad is None for exactly the frozen parameters, the prefix's running statistics
  and num_batches_tracked bitwise unchanged, net.stats filled.
* The switch with no prefix (n = 0) is bitwise the switch-off step; two forwards before one backward; optimizer steps do not
  re-pack, a changed prefix parameter does; net.logits(x) and the no-grad routes.
* 416x416, B=2, 80 classes, n = 52, F32 and BF16: the bitwise hand-over on the three routes (where F(4x4,3x3), the persistent 1x1
  GEMM and the real tile choices run)."""
import copy
import functools

import pytest
import torch

from tests import frozen_prefix_check as FC
from tests import test_gpu_train_bf16 as GB
from tests import test_gpu_train_local as L
from tests import train_states as S
from tests import yolo_loss_ref as R
from yolo_v3_amd import arch, backprop, F32, BF16, BF16_ACT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HW, C, B = (96, 96), 3, 2
MATHS = {"f32": F32, "bf16": BF16, "bf16_act": BF16_ACT}
NS = [52, 68, 8]


@functools.lru_cache(maxsize=None)
def inputs(seed=31):
    return L.images(B, HW, seed), R.random_rows(77 + seed, B, 8, C, (0.05, 0.7))


def make_net(state, math, on=True, hw=HW, num_class=C):
    net = state.apply(L.make_net(hw, num_class, math))
    net.frozen_prefix = on
    return net


@pytest.fixture
def handed(monkeypatch):
    """Every hand-over of the test, as the forward made it: [(run, bufs, bufs_b, logits)] right after backprop._prefix."""
    seen, real = [], backprop._prefix

    def spy(run, m, bufs, bufs_b, logits):
        real(run, m, bufs, bufs_b, logits)
        seen.append((run, dict(bufs), None if bufs_b is None else dict(bufs_b), list(logits)))
    monkeypatch.setattr(backprop, "_prefix", spy)
    return seen


def assert_hand_over(net, n, x, entry):
    """The hand-over `entry` of a forward on x: exactly HANDED[n]'s buffers, each bitwise the full inference engine's, in the reader's
    form, in memory of its own."""
    run, bufs, bufs_b, logits = entry
    mode = backprop.PREFIX_MODE[run.math]
    assert run.prefix == n and mode == (F32 if run.math == F32 else BF16)
    src, res, heads = FC.HANDED[n]
    Bx, _, H, W = x.shape
    peng = net.prefix_engine(mode, n)
    pplan = peng.plan(Bx, H, W, logits=True)
    assert peng.n_conv == n and len(peng.packed) == n and pplan.n_desc == n - 1 and not pplan.fused_decode
    plan_memory = {t.untyped_storage().data_ptr() for t in pplan._keep}
    full = net.engine(mode)
    _, plan = full.forward(x.to(DEV).float(), logits=True)
    torch.cuda.synchronize()
    assert plan is not pplan and full.n_conv == 75 and plan.n_desc == 74
    names = [sp.name for sp in arch.conv_specs(net.numClass)]
    if run.math == F32:
        assert bufs_b is None and set(bufs) == {"x"} | src | res | heads
    else:
        assert set(bufs_b) == src | res                                  # (no bf16 copy of x: the inference front reads x itself)
        assert set(bufs) == {"x"} | heads | (res if run.math == BF16 else set())
    for j, op in enumerate(run.ops[:n]):
        want = plan.layer_out[names[j]]
        assert run.shape[op.out] == (Bx,) + tuple(want.shape[-3:]) and run.need[op.out] is False, op.out
        got = []
        if op.out in heads:
            assert want.dtype == torch.float32 and logits[op.head_idx][0] is bufs[op.out]
            assert logits[op.head_idx][1:] == tuple(want.shape[1:3])
            assert torch.equal(bufs[op.out], want), op.out
            got.append(bufs[op.out])
        elif op.out in src | res and run.math == F32:
            assert bufs[op.out].dtype == torch.float32 and torch.equal(bufs[op.out], want), op.out
            got.append(bufs[op.out])
        elif op.out in src | res:
            assert want.dtype == torch.bfloat16 and want.shape[0] == 1
            assert bufs_b[op.out].dtype == torch.int16 and torch.equal(bufs_b[op.out], want[0].view(torch.int16)), op.out
            got.append(bufs_b[op.out])
            if op.out in bufs:                                           # BF16: the residual's fp32 copy, the exact widening
                assert bufs[op.out].dtype == torch.float32 and torch.equal(bufs[op.out], want[0].float()), op.out
                got.append(bufs[op.out])
        for t in got:
            assert t.is_contiguous() and t.untyped_storage().data_ptr() not in plan_memory, op.out
    assert all(logits[k] is not None for k in range(3)) == (n == 75)
    return peng, pplan


def prefix_owned(n, num_class=C):
    """state_dict keys of the first n convolutions' modules."""
    names = tuple(sp.name + "." for sp in arch.conv_specs(num_class)[:n])
    return lambda key: key.startswith(names)


# ---------------------------------------------------------------- one traced step per (math, cut)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("math", sorted(MATHS))
def test_one_step_with_a_prefix(math, n, handed):
    state = FC.CUTS[n]
    x, tg = inputs()
    net = make_net(state, MATHS[math])
    assert backprop.frozen_prefix_ops(net) == n
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    twin = copy.deepcopy(net)
    assert twin.frozen_prefix is True and twin._prefix_engines == {}
    net.stats = None
    run, loss, pg = L.traced_step(net, x, tg)
    assert len(handed) == 1 and handed[0][0] is run and run.prefix == n
    # ---- the hand-over is the inference engine, bitwise
    assert_hand_over(net, n, x, handed[0])
    # ---- state is untouched
    assert sorted(run.saved) == list(range(n, 75))
    owned = prefix_owned(n)
    after = net.state_dict()
    assert sum(owned(k) and k.endswith("running_var") for k in sd) == n - len(FC.HANDED[n][2])
    for k, v in sd.items():
        if owned(k):                                                     # parameters, running statistics, num_batches_tracked
            assert torch.equal(after[k].cpu(), v), k
    assert set(net.stats) == set(net.stat_keys) and net.stats["nGT"] > 0 and net.stats["loss"] > 0
    # ---- the training kernels are unchanged: ops >= n against float64 on the GPU's own inputs
    gone = handed[0][2] if MATHS[math] == BF16_ACT else None             # (BF16_ACT frees a bf16 buffer after its last reader)
    FC.check_from(n, net, sd, run, pg, state, "%s n=%d 96x96 B=2" % (math.upper(), n), gone)
    # ---- a plain step through net(x, target): bitwise the traced one, grad is None for exactly the frozen parameters
    l2 = GB.gpu_step(twin, x, tg)
    assert len(handed) == 2 and float(l2.detach()) == float(loss) and l2.requires_grad
    for (name, p), (_, q) in zip(net.named_parameters(), twin.named_parameters()):
        assert (q.grad is None) == (not state.trainable(name)) == (not q.requires_grad), name
        assert q.grad is None or torch.equal(q.grad, pg[id(p)].view_as(q)), name
    for (k, v), (_, v2) in zip(net.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(v, v2), k
    assert twin.stats == net.stats


# ---------------------------------------------------------------- the switch without a prefix
@pytest.mark.parametrize("math", sorted(MATHS))
@pytest.mark.parametrize("name", ["bn_frozen", "all_train"])
def test_switch_on_without_a_prefix_is_the_switch_off_step(name, math, handed):
    state = dict(S.STATES, all_train=S.ALL_TRAIN)[name]
    x, tg = inputs()
    on, off = make_net(state, MATHS[math]), make_net(state, MATHS[math], on=False)
    assert backprop.frozen_prefix_ops(on) == 0
    l_on, l_off = GB.gpu_step(on, x, tg), GB.gpu_step(off, x, tg)
    assert not handed and on._prefix_engines == {}
    assert torch.equal(l_on.detach(), l_off.detach()) and on.stats == off.stats
    for (k, p), (_, q) in zip(on.named_parameters(), off.named_parameters()):
        assert (p.grad is None) == (q.grad is None) == (not state.trainable(k)), k
        assert p.grad is None or torch.equal(p.grad, q.grad), k
    for (k, v), (_, v2) in zip(on.state_dict().items(), off.state_dict().items()):
        assert torch.equal(v, v2), k


# ---------------------------------------------------------------- copies, not aliases
@pytest.mark.parametrize("n", [52, 8])
@pytest.mark.parametrize("math", sorted(MATHS))
def test_two_forwards_before_one_backward(math, n):
    """The plan's buffers are overwritten by the second forward; the first step's backward still reads its own copies."""
    x1, t1 = inputs()
    x2, t2 = inputs(47)
    assert not torch.equal(x1, x2)
    a, b = make_net(FC.CUTS[n], MATHS[math]), make_net(FC.CUTS[n], MATHS[math])
    la = a(x1.to(DEV), torch.as_tensor(t1)) + a(x2.to(DEV), torch.as_tensor(t2))
    la.backward()
    l1 = b(x1.to(DEV), torch.as_tensor(t1))
    l1.backward()
    l2 = b(x2.to(DEV), torch.as_tensor(t2))
    l2.backward()
    torch.cuda.synchronize()
    assert float(la.detach()) == float((l1 + l2).detach())
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert (p.grad is None) == (q.grad is None) == (not FC.CUTS[n].trainable(k)), k
        assert p.grad is None or torch.equal(p.grad, q.grad), k
    for (k, v), (_, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(v, v2), k


# ---------------------------------------------------------------- the prefix engine's signature
@pytest.mark.parametrize("math", sorted(MATHS))
def test_optimizer_steps_do_not_repack_and_a_prefix_change_does(math, handed):
    n = 52
    x, tg = inputs()
    net = make_net(FC.CUTS[n], MATHS[math])
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-3)
    GB.gpu_step(net, x, tg)
    eng = net.prefix_engine(backprop.PREFIX_MODE[MATHS[math]], n)
    assert list(net._prefix_engines) == [(backprop.PREFIX_MODE[MATHS[math]], n)]
    gen, packed, plans = eng.generation, eng.packed, dict(eng._plans)
    assert gen == 1 and len(plans) == 1
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt.step()
    moved = [k for k, v in net.state_dict().items() if not torch.equal(v, before[k])]
    assert moved and not any(prefix_owned(n)(k) for k in moved)
    GB.gpu_step(net, x, tg)
    assert net.prefix_engine(eng.dtype, n) is eng and eng.generation == gen and eng.packed is packed
    assert list(eng._plans) == list(plans) and all(eng._plans[k] is p for k, p in plans.items())
    first, second = handed[0], handed[1]
    for d in (1, 2):                                                     # the same prefix on the same x: the same hand-over
        assert all(torch.equal(first[d][k], second[d][k]) for k in first[d] or ())
    with torch.no_grad():                                                # an in-place change of one prefix parameter
        net.feature.mlist[0].bn.bias.add_(0.05)
    GB.gpu_step(net, x, tg)
    assert eng.generation == gen + 1 and eng.packed is not packed and all(eng._plans[k] is not p for k, p in plans.items())
    third = handed[2]
    store = 1 if MATHS[math] == F32 else 2
    assert all(not torch.equal(first[store][k], third[store][k]) for k in FC.HANDED[n][0])
    assert_hand_over(net, n, x, third)                                   # ... and still the inference engine's
    net.repack()
    assert net._prefix_engines == {}


# ---------------------------------------------------------------- the other routes
def logits_step(net, x, tg):
    lg = net.logits(x.to(DEV))
    loss = sum(layer(lg[k], net.img_dim, torch.as_tensor(tg))[0] for k, layer in enumerate((net.yolo1, net.yolo2, net.yolo3)))
    loss.backward()
    torch.cuda.synchronize()
    return loss, lg


@pytest.mark.parametrize("math", sorted(MATHS))
def test_logits_route_gives_the_steps_gradients(math, handed):
    n = 52
    state = FC.CUTS[n]
    x, tg = inputs()
    a, b = make_net(state, MATHS[math]), make_net(state, MATHS[math])
    (la, lg), lb = logits_step(a, x, tg), GB.gpu_step(b, x, tg)
    assert len(handed) == 2 and handed[0][0].prefix == handed[1][0].prefix == n
    assert float(la.detach()) == float(lb.detach())
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert (p.grad is None) == (q.grad is None) == (not state.trainable(k)), k
        assert p.grad is None or torch.equal(p.grad, q.grad), k
    for (k, v), (_, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(v, v2), k
    # under torch.no_grad(): the same forward (the train-mode heads' running statistics move once more, on both nets alike)
    with torch.no_grad():
        lg2 = a.logits(x.to(DEV))
        l3 = b(x.to(DEV), torch.as_tensor(tg))
    torch.cuda.synchronize()
    assert len(handed) == 4 and handed[2][0].prefix == handed[3][0].prefix == n
    assert not l3.requires_grad and not any(t.requires_grad for t in lg2)
    for d in (1, 2):
        assert all(torch.equal(handed[0][d][k], handed[2][d][k]) for k in handed[0][d] or ())
    for (k, v), (_, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(v, v2), k


def test_a_fully_frozen_eval_net_runs_on_the_inference_engine_alone(handed):
    """n = 75: every op is a prefix op; the three heads hand over their logits and the loss is the inference path's."""
    x, tg = inputs()
    net = L.make_net(HW, C, F32).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    net.frozen_prefix = True
    assert backprop.frozen_prefix_ops(net) == 75
    loss = net(x.to(DEV), torch.as_tensor(tg))
    torch.cuda.synchronize()
    run, bufs, bufs_b, logits = handed[0]
    assert run.prefix == 75 and not run.saved and not loss.requires_grad and sorted(bufs) == sorted(["x"] + [op.out for op in run.ops if op.head])
    stats = dict(net.stats)
    net.backprop, net.math_mode = False, F32                             # net._loss: the full F32 engine's logits plan
    l2 = net(x.to(DEV), torch.as_tensor(tg))
    assert float(loss) == float(l2) and stats == net.stats


# ---------------------------------------------------------------- 416x416, 80 classes: the hand-over at real shapes
@pytest.mark.parametrize("math", ["f32", "bf16"])
def test_hand_over_at_416_on_the_three_routes(math, handed):
    n, hw, nc = 52, (416, 416), 80
    net = make_net(FC.CUTS[n], MATHS[math], hw=hw, num_class=nc)
    assert backprop.frozen_prefix_ops(net) == n
    x = L.images(B, hw, 511).to(DEV)
    tg = torch.as_tensor(R.random_rows(588, B, 20, nc, (0.05, 0.7)))
    loss = net(x, tg)
    lg = net.logits(x)
    with torch.no_grad():
        net(x, tg)
    torch.cuda.synchronize()
    assert loss.requires_grad and all(t.requires_grad for t in lg) and len(handed) == 3
    engines = set()
    for entry in handed:
        peng, _ = assert_hand_over(net, n, x, entry)
        engines.add(id(peng))
    assert len(engines) == 1 and peng.generation == 1                    # one engine, packed once, for the three routes
    del loss, lg
