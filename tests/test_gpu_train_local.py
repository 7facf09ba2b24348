"""Every op of a real training step against float64 *on the inputs the GPU fed it* (yolo_v3_amd/backprop.py; csrc/train.hip,
csrc/train_bf16.hip), plus the first rectangular whole steps.

The whole-step tests (tests/test_gpu_train.py, test_gpu_train_bf16.py) bound each tensor by 16x the worst tensor of a torch-fp32 CPU
run: the right yardstick for an ill-conditioned 75-layer train-mode step, and loose by construction.  Here one step runs through
backprop.forward / backprop.backward with the trace on (_Run.trace), and each of the 75 ops of backprop.graph(net) is restated alone
in float64 (tests/train_kernel_ref.py) from the tensors the GPU held at that point -- forward: z, the statistics, the output buffer;
backward: dz, dgamma / dbeta / dbias, dw and what the op added to the gradient of each of its inputs.  The errors do not compound, so
the bars are the kernels' own: CONV_BAR * sum|a||b| for conv products, BN_BAR of the largest reference magnitude for elementwise /
per-channel results, with the kink rule for the BN backward (undecided share <= KINK_SHARE over the step).  The graph's wiring is
checked with it: the dy an op receives is bitwise the buffer the last of its consumers left, every buffer got as many contributions
as it has consumers, and a step with the trace off gives bitwise the same gradients and running statistics."""
import copy

import numpy as np
import pytest
import torch

from tests import test_gpu_train as G
from tests import test_gpu_train_bf16 as GB
from tests import train_kernel_ref as K
from tests import train_ref as T
from tests import train_ref_bf16 as TB
from tests import train_states as S
from tests import yolo_loss_ref as R
from tests.helpers import trained_like_stream
from yolo_v3_amd import YoloNet, WeightManager, backprop, synth, F32, BF16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_net(hw, C, math):
    net = YoloNet(hw, numClass=C)
    WeightManager(net).load_stream(trained_like_stream(C))
    net = net.to(DEV)
    net.backprop, net.backprop_math = True, math
    return net


def images(B, hw, seed):
    """Synthetic scenes of height x width hw (a crop of the square scene of the larger side)."""
    return torch.from_numpy(np.ascontiguousarray(synth.images(B, max(hw), seed)[:, :, :hw[0], :hw[1]]))


def nchw64(t):
    """An NHWC fp32 GPU buffer -> NCHW float64 on the CPU."""
    return t.detach().cpu().double().permute(0, 3, 1, 2)


class Worst:
    """Worst error / bar ratio per kind of result, with the op it came from."""

    def __init__(self):
        self.w = {}

    def add(self, kind, where, r):
        if r > self.w.get(kind, (-1.0, None))[0]:
            self.w[kind] = (r, where)

    def report(self, what):
        print("%s: worst error / bar per result (op):" % what, {k: "%.3g (%s)" % v for k, v in sorted(self.w.items())})
        bad = {k: v for k, v in self.w.items() if not v[0] <= 1.0}
        assert not bad, bad


def traced_step(net, x, tg):
    """One step through backprop.forward / backward with the trace on -> (run, loss, {id(param): grad})."""
    run = backprop._Run(net, x.to(DEV).float().contiguous(), torch.as_tensor(tg), backprop.backprop_math(net))
    run.trace = {}
    with torch.no_grad():
        loss = backprop.forward(run, want_grad=True)
        pg = backprop.backward(run, torch.ones((), device=DEV))
    torch.cuda.synchronize()
    return run, loss, pg


def check_step(net, sd, run, pg, train, what, state=None):
    """Each op of the traced step against float64 on the GPU's own inputs; sd: the state_dict before the step.  With a `state`
    (tests/train_states.py) it, not `train`, gives each op's BatchNorm mode, momentum and eps, and the ops the walk visits and what
    each does there must be exactly tests/train_states.py's expected_walk."""
    bf = run.math == BF16
    r = K.rb if bf else (lambda t: t)
    ops, keys = run.ops, K.op_params(net, run.ops)
    bufs, tr = run.bufs, run.trace
    walk = S.expected_walk(state if state is not None else S.ALL_TRAIN, ops)
    assert state is not None or all(v is not None for v in walk.values())
    assert sorted(tr) == [i for i in range(len(ops)) if walk[i] is not None]

    def bn_of(kbn):
        """(training, the batch's weight in the running statistics, eps) of one op's BatchNorm."""
        return (train, K.MOMENTUM, K.EPS) if state is None else (state.bn(kbn)[0], state.factor(kbn), state.bn(kbn)[2])

    P = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}       # parameters (unchanged) and the new running stats
    before = {k: v.detach().cpu().double() for k, v in sd.items()}
    w = Worst()
    cpu = {"x": bufs["x"].detach().cpu().double()}

    def buf64(name):
        if name not in cpu:
            cpu[name] = nchw64(bufs[name])
        return cpu[name]

    def conv_in(op):
        return buf64(op.src) if op.src2 is None else K.upcat(buf64(op.src2), buf64(op.src))

    if bf:                                                  # the bf16 copies: bitwise the fp32 buffers rounded by torch
        assert sorted(run.bufs_b) == sorted(n for n in bufs if not n.endswith(".logits"))
        for name, tb in run.bufs_b.items():
            assert torch.equal(tb.view(-1), bufs[name].to(torch.bfloat16).view(torch.int16).view(-1)), name
    # ---- forward
    stats = {}
    for i, (op, (kw, kb, kbn)) in enumerate(zip(ops, keys)):
        st = op.conv.stride[0]
        xin = r(conv_in(op))
        z_gpu = bufs[op.out] if op.head else run.saved[i]["z"]
        ref, sc = K.conv_fwd(xin, r(P[kw]), st, P[kb] if kb else None)
        w.add("z", op.out, K.conv_ratio(nchw64(z_gpu), ref, sc))
        if op.head:
            continue
        sv = run.saved[i]
        zr = K.rows(nchw64(z_gpu))
        mean_g, invstd_g = sv["mean"].cpu().double(), sv["invstd"].cpu().double()
        training, mom, eps = bn_of(kbn)
        if training:
            mean, var, invstd = K.bn_batch_stats(zr, eps)
            rm, rv = K.bn_running(mean, var, zr.shape[0], before[kbn + ".running_mean"], before[kbn + ".running_var"], mom)
            w.add("mean", op.out, K.bn_ratio(mean_g, mean))
            w.add("running_mean", op.out, K.bn_ratio(P[kbn + ".running_mean"], rm))
            w.add("running_var", op.out, K.bn_ratio(P[kbn + ".running_var"], rv))
        else:
            _, invstd = K.bn_eval_stats(before[kbn + ".running_mean"], before[kbn + ".running_var"], eps)
            assert torch.equal(mean_g, before[kbn + ".running_mean"]), op.out
            assert torch.equal(P[kbn + ".running_mean"], before[kbn + ".running_mean"]), op.out
            assert torch.equal(P[kbn + ".running_var"], before[kbn + ".running_var"]), op.out
        w.add("invstd", op.out, K.bn_ratio(invstd_g, invstd))
        res = K.rows(buf64(op.res)) if op.res is not None else None
        y = K.bn_act_fwd(zr, mean_g, invstd_g, P[kbn + ".weight"], P[kbn + ".bias"], res)
        w.add("y", op.out, K.bn_ratio(K.rows(buf64(op.out)), y))
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
            last[op.out], count[op.out] = run.dlogits[op.head_idx], 0
            consumers[op.out] = 0

    def contribute(buf, after):
        last[buf], count[buf] = after, count.get(buf, 0) + 1

    named = dict(net.named_parameters())
    und = total = 0
    want_pg = set()
    for i in range(len(ops) - 1, -1, -1):
        if walk[i] is None:                                            # not needed: no contribution may have reached it either
            assert ops[i].head or ops[i].out not in count, ops[i].out
            continue
        op, (kw, kb, kbn), t = ops[i], keys[i], tr[i]
        assert set(t) & set(S.WALK_KEYS) == walk[i], (op.out, sorted(t), sorted(walk[i]))
        mine = ([kb] if op.head else [kbn + ".weight", kbn + ".bias"]) + ([kw] if "dw" in walk[i] else [])
        want_pg.update(id(named[k]) for k in mine)
        st = op.conv.stride[0]
        assert count[op.out] == consumers[op.out], (op.out, count[op.out], consumers[op.out])
        assert torch.equal(t["dy"], last[op.out]), op.out              # the dy the op got is what its consumers left
        dy = nchw64(t["dy"])
        B, _, Ho, Wo = dy.shape
        if op.head:
            assert torch.equal(t["dz"], t["dy"]), op.out               # dL/dloss = 1: one exact fp32 multiply
            _, db, da = K.bias_bwd(K.rows(dy))
            w.add("dbias", op.out, K.ratio(t["dbias"], db, K.BN_BAR * da + 1e-30))
            assert pg[id(named[kb])] is not None and torch.equal(pg[id(named[kb])], t["dbias"])
        else:
            zr, mean_g, invstd_g = stats[i]
            b = K.bn_act_bwd(zr, K.rows(dy), mean_g, invstd_g, P[kbn + ".weight"], P[kbn + ".bias"], bn_of(kbn)[0])
            und, total = und + int(b["und"].sum()), total + b["und"].numel()
            for k_, v in K.bn_bwd_ratios(K.rows(nchw64(t["dz"])), t["dgamma"], t["dbeta"], b).items():
                w.add(k_, op.out, v)
            assert torch.equal(pg[id(named[kbn + ".weight"])], t["dgamma"]) and torch.equal(pg[id(named[kbn + ".bias"])], t["dbeta"])
            if "res_after" in walk[i]:
                want = t["dy"] if "res_before" not in t else (t["res_before"].double() + t["dy"].double()).float()
                assert torch.equal(t["res_after"], want), op.out       # one fp32 add per element: exact
                contribute(op.res, t["res_after"])
        dz = r(nchw64(t["dz"]))
        xin = r(conv_in(op))
        if "dw" in walk[i]:
            ref, sc = K.conv_wgrad(xin, P[kw].shape, dz, st)
            w.add("dw", op.out, K.conv_ratio(t["dw"], ref, sc))
            assert torch.equal(pg[id(named[kw])].view_as(t["dw"]), t["dw"])
        if op.src == "x":
            assert "dx_after" not in t and "dcat" not in t
            continue
        if not walk[i] & {"dx_after", "dcat"}:                         # no input is needed: no dgrad ran
            continue
        ref, sc = K.conv_dgrad(xin.shape, r(P[kw]), dz, st)
        if op.cin_up == 0:
            if "dx_before" in t:
                base = nchw64(t["dx_before"])
                ref, sc = ref + base, sc + base.abs()
            w.add("dx" + ("+=" if "dx_before" in t else ""), op.out, K.conv_ratio(nchw64(t["dx_after"]), ref, sc))
            contribute(op.src, t["dx_after"])
        else:
            w.add("dcat", op.out, K.conv_ratio(nchw64(t["dcat"]), ref, sc))
            rl, sl, rt = K.upcat_bwd(nchw64(t["dcat"]), op.cin_up)
            if "dlow_before" in t:
                base = nchw64(t["dlow_before"])
                rl, sl = rl + base, sl + base.abs()
            if "dlow_after" in walk[i]:
                w.add("dlow", op.out, K.ratio(nchw64(t["dlow_after"]), rl, K.BN_BAR * sl + 1e-30))
                contribute(op.src2, t["dlow_after"])
            if "dtail_after" in walk[i]:
                if "dtail_before" in t:
                    rt = (nchw64(t["dtail_before"]) + rt).float().double()
                assert torch.equal(nchw64(t["dtail_after"]), rt), op.out   # a copy or one fp32 add: exact
                contribute(op.src, t["dtail_after"])
    assert set(pg) == want_pg                                          # exactly the gradients of the walked ops' parameters
    if state is None:
        assert len(pg) == len(named) == 75 + 2 * 72 + 3
    share = und / max(total, 1)
    print("%s: %d of %d BN elements undecided at the kink (%.3g)" % (what, und, total, share))
    assert share <= K.KINK_SHARE
    w.report(what)


def untraced_twin_agrees(twin, x, tg, net, loss, pg):
    """A plain step (trace off) on a copy of the net: bitwise the traced step's loss, gradients and state."""
    l2 = GB.gpu_step(twin, x, tg)
    assert float(l2.detach()) == float(loss)
    for (n1, p1), (n2, p2) in zip(net.named_parameters(), twin.named_parameters()):
        assert n1 == n2 and p2.grad is not None and torch.equal(p2.grad, pg[id(p1)].view_as(p2)), n1
    for (k1, v1), (_, v2) in zip(net.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(v1, v2), k1


def run_local_case(hw, C, B, train, math, seed, rows=8):
    net = make_net(hw, C, math).train(train)
    x = images(B, hw, seed)
    tg = R.random_rows(77 + seed, B, rows, C, (0.05, 0.7))
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    twin = copy.deepcopy(net)
    run, loss, pg = traced_step(net, x, tg)
    assert sorted(run.trace) == list(range(75))
    untraced_twin_agrees(twin, x, tg, net, loss, pg)
    check_step(net, sd, run, pg, train, "%dx%d B=%d C=%d %s %s" % (hw[0], hw[1], B, C, "train" if train else "eval",
                                                                    "BF16" if math == BF16 else "F32"))


@pytest.mark.parametrize("math", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hw,train", [((96, 96), True), ((96, 96), False), ((96, 160), True)], ids=["96x96-train", "96x96-eval", "96x160-train"])
def test_every_op_against_float64_on_the_gpu_inputs(hw, train, math):
    run_local_case(hw, 3, 2, train, math, 31)


def test_every_op_against_float64_on_the_gpu_inputs_416():
    run_local_case((416, 416), 80, 1, True, F32, 511, rows=20)


def test_trace_is_off_by_default():
    net = make_net((96, 96), 3, F32)
    assert backprop._Run(net, torch.zeros(1, 3, 96, 96), torch.zeros(1, 1, 5)).trace is None


# ---------------------------------------------------------------- the first rectangular whole steps (the loss takes img_dim from H)
def _rect_step(math, ref_mod, check):
    hw, C, B = (96, 160), 3, 2
    net = make_net(hw, C, math).train()
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = images(B, hw, 47)
    logits, _, _ = ref_mod.forward(sd, x, True)
    assert [tuple(l.shape[2:]) for l in logits] == [(3, 5), (6, 10), (12, 20)]
    tg = None
    for attempt in range(100):                      # a target draw whose decisions clear the reference's margins (as pick_target)
        cand = R.random_rows(61000 + attempt, B, 8, C, (0.05, 0.7), n_valid_lo=3)
        res = T.head_losses(logits, cand, hw[0], C)
        if all(R.margins_ok(r_["margins"]) for r_ in res) and sum(r_["nGT"] for r_ in res) > 0:
            tg = cand
            break
    assert tg is not None
    loss = GB.gpu_step(net, x, tg)
    check(sd, net, loss, x, tg, C, True)


def test_rectangular_step_matches_float64_f32():
    _rect_step(F32, T, G.check_against_ref)


def test_rectangular_step_matches_float64_bf16():
    _rect_step(BF16, TB, GB.check_against_ref)
