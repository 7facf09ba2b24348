"""Whole BF16_ACT training steps (net.backprop_math = BF16_ACT; yolo_v3_amd/backprop.py) against the float64 restatement
tests/train_ref_bf16_act.py, op by op on the tensors the GPU fed each op (_Run.trace), the bitwise equivalences of the training path,
and the memory a step holds between forward and backward.

Bars.  Whole steps compare every parameter gradient, running statistic, the loss and x.grad by relative L2 against the float64 step;
the bar is BAR_FACTOR times the largest error the same restatement shows in dtype=float32 on the CPU on the same case.  The yardstick
is measured because a stored rounding flips when fp32 and float64 land on different sides of a bf16 boundary, and the CPU fp32 run
flips at the same rate.  Op by op the bars are those of tests/test_gpu_train_bf16_act.py: fp32 results as the fp32 kernels', a bf16
result |out - ref| <= 2^-8 |ref| plus the fp32 bar of the same result."""
import functools
import gc

import pytest
import torch

from tests import test_gpu_train_bf16 as GB
from tests import test_gpu_train_local as L
from tests import train_kernel_ref as K
from tests import train_ref_bf16_act as TA
from tests import yolo_loss_ref as R
from tests.test_gpu_train_bf16_act import U, b16_ratio
from yolo_v3_amd import backprop, BF16, BF16_ACT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, B = 3, 2
BAR_FACTOR = 16.0


def make_net(hw, train=True, math=BF16_ACT, frozen=False, input_grad=False):
    net = L.make_net(hw, C, math).train(train)
    net.input_grad = input_grad
    if frozen:
        for n, p in net.named_parameters():
            if n.startswith("feature."):
                p.requires_grad_(False)
    return net


@functools.lru_cache(maxsize=None)
def case(hw, train, frozen):
    """(state_dict, x, target, float64 step, fp32 CPU step) -- computed once per case and left unchanged."""
    net = make_net(hw, train)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = L.images(B, hw, 31)
    logits, _, _ = TA.forward(sd, x, train)
    tg = GB.pick_target(logits, hw[0], C, B, 8, 77)
    want_x = hw == (96, 96) and train and not frozen
    ref = TA.run(sd, x, tg, C, train=train, frozen_backbone=frozen, x_requires_grad=want_x)
    ref32 = TA.run(sd, x, tg, C, train=train, dtype=torch.float32, frozen_backbone=frozen, x_requires_grad=want_x)
    return sd, x, tg, ref, ref32


def check_against_ref(net, loss, ref, ref32, train, xgrad=None):
    """`train`: the mode of every BatchNorm, or a function of the conv_bn_relu prefix where they differ."""
    train_of = train if callable(train) else (lambda prefix: train)
    assert net.stats["nGT"] == ref["stats"][8] and abs(net.stats["nCorrect"] - ref["stats"][7]) <= 1
    worst = [("loss", abs(float(loss.detach()) - ref["loss"]) / abs(ref["loss"]), abs(ref32["loss"] - ref["loss"]) / abs(ref["loss"]))]
    named = dict(net.named_parameters())
    for k, g64 in ref["grads"].items():
        if k == "x" and xgrad is None:
            continue
        g = xgrad if k == "x" else named[k].grad
        if g64 is None:
            assert g is None, k
            continue
        assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all(), k
        worst.append((k, TA.rel_l2(g.cpu(), g64), TA.rel_l2(ref32["grads"][k], g64)))
    mods = dict(net.named_modules())
    for prefix, (m64, v64) in ref["running"].items():
        bn = mods[prefix].bn
        if not train_of(prefix):
            assert torch.equal(bn.running_mean.cpu().double(), m64) and torch.equal(bn.running_var.cpu().double(), v64), prefix
            continue
        worst.append((prefix + ".running_mean", TA.rel_l2(bn.running_mean.cpu(), m64), TA.rel_l2(ref32["running"][prefix][0], m64)))
        worst.append((prefix + ".running_var", TA.rel_l2(bn.running_var.cpu(), v64), TA.rel_l2(ref32["running"][prefix][1], v64)))
    bar = BAR_FACTOR * max(e32 for _, _, e32 in worst)
    worst.sort(key=lambda t: -t[1])
    print("bar %.3g = %g x the fp32 CPU step's worst error; worst GPU error / bar %.3g; largest GPU errors (tensor, GPU, fp32 CPU):"
          % (bar, BAR_FACTOR, worst[0][1] / bar), [(k, "%.3g" % e, "%.3g" % e32) for k, e, e32 in worst[:4]])
    assert worst[0][1] <= bar, (bar, worst[:4])


# ---------------------------------------------------------------- whole steps against the float64 restatement
@pytest.mark.parametrize("hw,train,frozen", [((96, 96), True, False), ((96, 96), False, False), ((96, 160), True, False), ((96, 96), True, True)],
                         ids=["96x96-train", "96x96-eval", "96x160-train", "96x96-frozen-backbone"])
def test_step_matches_float64(hw, train, frozen):
    sd, x, tg, ref, ref32 = case(hw, train, frozen)
    net = make_net(hw, train, frozen=frozen)
    loss = GB.gpu_step(net, x, tg)
    assert loss.requires_grad
    check_against_ref(net, loss, ref, ref32, train)
    assert int(net.feature.mlist[0].bn.num_batches_tracked) == (1 if train else 0)
    if frozen:
        assert all((p.grad is None) == n.startswith("feature.") for n, p in net.named_parameters())


def test_input_grad_matches_float64_and_changes_nothing_else():
    sd, x, tg, ref, ref32 = case((96, 96), True, False)
    on, off = make_net((96, 96), input_grad=True), make_net((96, 96))
    xd = x.to(DEV).requires_grad_(True)
    l_on = on(xd, torch.as_tensor(tg))
    l_on.backward()
    l_off = GB.gpu_step(off, x, tg)
    torch.cuda.synchronize()
    assert xd.grad is not None and tuple(xd.grad.shape) == tuple(x.shape)
    check_against_ref(on, l_on, ref, ref32, True, xgrad=xd.grad)
    assert float(l_on.detach()) == float(l_off.detach())
    for (n, p), (_, q) in zip(on.named_parameters(), off.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    for (k, v), (_, v2) in zip(on.state_dict().items(), off.state_dict().items()):
        assert torch.equal(v, v2), k
    with pytest.raises(NotImplementedError):
        off(x.to(DEV).requires_grad_(True), torch.as_tensor(tg))


# ---------------------------------------------------------------- bitwise equivalences
def _same(a, b):
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), n
    for (k, v), (_, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(v, v2), k


def test_two_identical_steps_give_identical_bits():
    _, x, tg, _, _ = case((96, 96), True, False)
    a, b = make_net((96, 96)), make_net((96, 96))
    la, lb = GB.gpu_step(a, x, tg), GB.gpu_step(b, x, tg)
    assert float(la) == float(lb)
    _same(a, b)
    bf = make_net((96, 96), math=BF16)                       # and the mode is not BF16 under another name
    GB.gpu_step(bf, x, tg)
    assert any(not torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), bf.parameters()))


def test_yolo_layers_on_logits_are_the_training_step():
    _, x, tg, _, _ = case((96, 96), True, False)
    tgt = torch.as_tensor(tg)
    a, b = make_net((96, 96)), make_net((96, 96))
    xd = x.to(DEV)
    lg = a.logits(xd)
    assert all(l.dtype == torch.float32 for l in lg)
    la = sum(head(l, a.img_dim, tgt)[0] for head, l in zip((a.yolo1, a.yolo2, a.yolo3), lg))
    la.backward()
    lb = b(xd, tgt)
    lb.backward()
    torch.cuda.synchronize()
    assert float(la.detach()) == float(lb.detach())
    _same(a, b)
    with torch.no_grad():                                    # the no-grad loss is the forward of the step
        c = make_net((96, 96))
        assert float(c(xd, tgt)) == float(lb.detach()) and all(p.grad is None for p in c.parameters())
        _same_state = [torch.equal(v, v2) for v, v2 in zip(c.state_dict().values(), b.state_dict().values())]
        assert all(_same_state)


def test_gradients_accumulate_and_scale():
    _, x, tg, _, _ = case((96, 96), True, False)
    a, b = make_net((96, 96), train=False), make_net((96, 96), train=False)
    xd, tgt = x.to(DEV), torch.as_tensor(tg)
    a(xd, tgt).backward()
    a(xd, tgt).backward()                                    # .grad += the same gradient: exactly twice it
    b(xd, tgt).backward(torch.tensor(2.0, device=DEV))
    torch.cuda.synchronize()
    one = make_net((96, 96), train=False)
    one(xd, tgt).backward()
    for (n, p), (_, q) in zip(a.named_parameters(), one.named_parameters()):
        assert torch.equal(p.grad, q.grad * 2), n
    worst = max(TA.rel_l2(p.grad.cpu(), q.grad.cpu() * 2) for p, q in zip(b.parameters(), one.parameters()))
    assert worst <= 2.0 ** -7, worst                         # (dL/dloss = 2 enters before dz is rounded: bf16-level agreement)


# ---------------------------------------------------------------- every op of a traced step on the GPU's own inputs
def b16(t):
    """int16 bf16 bits (GPU) -> float64 values (CPU), same shape."""
    return t.detach().cpu().view(torch.bfloat16).double()


def nchw(t, shape):
    """A flat or NHWC bf16 / fp32 GPU buffer of NHWC `shape` -> NCHW float64 on the CPU."""
    v = b16(t) if t.dtype == torch.int16 else t.detach().cpu().double()
    return v.reshape(shape).permute(0, 3, 1, 2)


def traced_step(net, x, tg):
    run = backprop._Run(net, x.to(DEV).float().contiguous(), torch.as_tensor(tg), backprop.backprop_math(net))
    run.trace = {}
    with torch.no_grad():
        loss = backprop.forward(run, want_grad=True)
        pg = backprop.backward(run, torch.ones((), device=DEV))
    torch.cuda.synchronize()
    return run, loss, pg


def test_every_op_against_float64_on_the_gpu_inputs():
    _, x, tg, _, _ = case((96, 96), True, False)
    net, twin = make_net((96, 96)), make_net((96, 96))
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    run, loss, pg = traced_step(net, x, tg)
    assert sorted(run.trace) == list(range(75))
    L.untraced_twin_agrees(twin, x, tg, net, loss, pg)       # tracing changes no bit
    ops, keys, tr, shape = run.ops, K.op_params(net, run.ops), run.trace, run.shape
    P = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    # fp32 exists only for x and the head logits; every activation is one bf16 tensor
    assert sorted(run.bufs) == sorted(["x"] + [op.out for op in ops if op.head])
    assert all(t.dtype == torch.float32 for t in run.bufs.values())
    assert sorted(run.bufs_b) == sorted(["x"] + [op.out for op in ops if not op.head])
    assert all(t.dtype == torch.int16 for t in run.bufs_b.values())
    assert torch.equal(run.bufs_b["x"], run.bufs["x"].to(torch.bfloat16).view(torch.int16).view(-1))
    w = L.Worst()
    cpu = {"x": b16(run.bufs_b["x"]).reshape(run.bufs["x"].shape)}

    def act(name):
        if name not in cpu:
            cpu[name] = nchw(run.bufs_b[name], shape[name])
        return cpu[name]

    def conv_in(op):
        return act(op.src) if op.src2 is None else K.upcat(act(op.src2), act(op.src))

    stats = {}
    for i, (op, (kw, kb, kbn)) in enumerate(zip(ops, keys)):
        st = op.conv.stride[0]
        ref, sc = K.conv_fwd(conv_in(op), K.rb(P[kw]), st, P[kb] if kb else None)
        if op.head:
            w.add("logits", op.out, K.conv_ratio(L.nchw64(run.bufs[op.out]), ref, sc))
            continue
        sv = run.saved[i]
        assert sv["z"].dtype == torch.int16
        zb = nchw(sv["z"], shape[op.out])
        w.add("zb", op.out, K.ratio(zb, ref, U * ref.abs() + K.CONV_BAR * sc + 1e-30))
        zr = K.rows(zb)
        mean_g, invstd_g = sv["mean"].cpu().double(), sv["invstd"].cpu().double()
        mean, var, invstd = K.bn_batch_stats(zr)
        rm, rv = K.bn_running(mean, var, zr.shape[0], sd[kbn + ".running_mean"], sd[kbn + ".running_var"])
        w.add("mean", op.out, K.bn_ratio(mean_g, mean))
        w.add("invstd", op.out, K.bn_ratio(invstd_g, invstd))
        w.add("running_mean", op.out, K.bn_ratio(P[kbn + ".running_mean"], rm))
        w.add("running_var", op.out, K.bn_ratio(P[kbn + ".running_var"], rv))
        res = K.rows(act(op.res)) if op.res is not None else None
        y = K.bn_act_fwd(zr, mean_g, invstd_g, P[kbn + ".weight"], P[kbn + ".bias"], res)
        w.add("y", op.out, b16_ratio(K.rows(act(op.out)), y))
        stats[i] = (zr, mean_g, invstd_g)
    # ---- backward, in the order the graph runs it
    consumers = {}
    for op in ops:
        for b in (op.src, op.src2, op.res):
            if b is not None and b != "x":
                consumers[b] = consumers.get(b, 0) + 1
    last, count = {}, {}
    for op in ops:
        if op.head:
            last[op.out], count[op.out], consumers[op.out] = run.dlogits[op.head_idx], 0, 0

    def contribute(buf, after):
        last[buf], count[buf] = after, count.get(buf, 0) + 1

    named = dict(net.named_parameters())
    und = total = 0
    for i in range(len(ops) - 1, -1, -1):
        op, (kw, kb, kbn), t = ops[i], keys[i], tr[i]
        st = op.conv.stride[0]
        assert count[op.out] == consumers[op.out], (op.out, count[op.out], consumers[op.out])
        assert t["dy"].dtype == torch.float32 and torch.equal(t["dy"], last[op.out]), op.out     # what its consumers left, bitwise
        dy = L.nchw64(t["dy"])
        Bn, cout, Ho, Wo = dy.shape
        cp = (cout + 7) // 8 * 8
        assert t["dz"].dtype == torch.int16 and t["dz"].numel() == Bn * Ho * Wo * cp
        dzp = t["dz"].view(Bn, Ho, Wo, cp)
        assert not bool(dzp[..., cout:].any()), op.out                                           # the padding channels are zero
        dz = nchw(dzp[..., :cout].contiguous(), (Bn, Ho, Wo, cout))
        if op.head:
            assert torch.equal(dzp[..., :cout], t["dy"].to(torch.bfloat16).view(torch.int16)), op.out   # dL/dloss = 1: a pure cast
            _, db, da = K.bias_bwd(K.rows(dy))
            w.add("dbias", op.out, K.ratio(t["dbias"], db, K.BN_BAR * da + 1e-30))
            assert torch.equal(pg[id(named[kb])], t["dbias"])
        else:
            zr, mean_g, invstd_g = stats[i]
            b = K.bn_act_bwd(zr, K.rows(dy), mean_g, invstd_g, P[kbn + ".weight"], P[kbn + ".bias"], True)
            und, total = und + int(b["und"].sum()), total + b["und"].numel()
            w.add("dz", op.out, b16_ratio(K.rows(dz), b["dz"], b["dz_growth"], b["und"]))
            w.add("dgamma", op.out, K.bn_ratio(t["dgamma"], b["dgamma"], b["S"]))
            w.add("dbeta", op.out, K.bn_ratio(t["dbeta"], b["dbeta"], b["S"]))
            assert torch.equal(pg[id(named[kbn + ".weight"])], t["dgamma"]) and torch.equal(pg[id(named[kbn + ".bias"])], t["dbeta"])
            if op.res is not None:
                want = t["dy"] if "res_before" not in t else (t["res_before"].double() + t["dy"].double()).float()
                assert torch.equal(t["res_after"], want), op.out
                contribute(op.res, t["res_after"])
        xin = conv_in(op)
        ref, sc = K.conv_wgrad(xin, P[kw].shape, dz, st)
        w.add("dw", op.out, K.conv_ratio(t["dw"], ref, sc))
        assert torch.equal(pg[id(named[kw])].view_as(t["dw"]), t["dw"])
        if op.src == "x":
            continue
        ref, sc = K.conv_dgrad(xin.shape, K.rb(P[kw]), dz, st)
        if op.cin_up == 0:
            if "dx_before" in t:
                base = L.nchw64(t["dx_before"])
                ref, sc = ref + base, sc + base.abs()
            w.add("dx", op.out, K.conv_ratio(L.nchw64(t["dx_after"]), ref, sc))
            contribute(op.src, t["dx_after"])
        else:
            w.add("dcat", op.out, K.conv_ratio(L.nchw64(t["dcat"]), ref, sc))
            contribute(op.src2, t["dlow_after"])
            contribute(op.src, t["dtail_after"])
    assert len(pg) == len(named) == 75 + 2 * 72 + 3
    share = und / max(total, 1)
    print("BF16_ACT 96x96: %d of %d BN elements undecided at the kink (%.3g)" % (und, total, share))
    assert share <= K.KINK_SHARE
    w.report("BF16_ACT 96x96 B=2 train")


def test_a_frozen_backbone_keeps_no_backbone_activation():
    _, x, tg, _, _ = case((96, 96), True, True)
    net = make_net((96, 96), frozen=True)
    run = backprop._Run(net, x.to(DEV).float().contiguous(), torch.as_tensor(tg), BF16_ACT)
    with torch.no_grad():
        backprop.forward(run, want_grad=True)
    torch.cuda.synchronize()
    r36, r61 = "f%d" % net.feature.map2yolocfg[36], "f%d" % net.feature.map2yolocfg[61]
    last = [n for n in run.bufs_b if n.startswith("f")]
    assert sorted(last) == sorted({r36, r61, run.ops[[op.out for op in run.ops].index("pre_det1.0")].src}), last
    for i, op in enumerate(run.ops):
        if not op.head:
            assert (run.saved[i]["z"] is None) == op.out.startswith("f"), op.out


# ---------------------------------------------------------------- memory held between forward and backward
def held_bytes(math, batch):
    net = make_net((96, 96), math=math)
    x = L.images(batch, (96, 96), 31).to(DEV)
    tg = torch.as_tensor(R.random_rows(5, batch, 8, C, (0.05, 0.7)))
    torch.cuda.synchronize()
    gc.collect()
    before = torch.cuda.memory_allocated()
    loss = net(x, tg)
    held = torch.cuda.memory_allocated() - before
    loss.backward()
    torch.cuda.synchronize()
    return held


def test_activations_take_at_most_045_of_the_bf16_steps_memory():
    """Per activation element BF16 holds fp32 z, fp32 y and the bf16 copy of y (10 bytes), BF16_ACT zb and y in bf16 (4): 0.40; the
    head logits and their gradient, equal in both modes, add about 2 %.  The difference between two batch sizes cancels the per-step
    weight images, which dwarf the activations at this size."""
    m = {(math, b): held_bytes(math, b) for math in (BF16, BF16_ACT) for b in (2, 4)}
    d_bf, d_act = m[BF16, 4] - m[BF16, 2], m[BF16_ACT, 4] - m[BF16_ACT, 2]
    print("held bytes (math, batch):", {("BF16_ACT" if k[0] == BF16_ACT else "BF16", k[1]): v for k, v in m.items()},
          "per 2 images: BF16 %d, BF16_ACT %d, ratio %.3f" % (d_bf, d_act, d_act / d_bf))
    assert d_bf > 0 and d_act > 0
    assert d_act <= 0.45 * d_bf
