"""The states and the checker of the frozen-prefix tests (net.frozen_prefix; tests/test_frozen_prefix_host.py,
tests/test_gpu_frozen_prefix.py).

The states: the three cuts the tests run, each a tests/train_states.State so that expected_walk and the float64 restatements apply.

``check_from(n, ...)`` restates tests/test_gpu_train_local.check_step for the ops from n on, in the three math modes: each op of a
traced step against float64 on the inputs the GPU fed it -- z, the statistics, y, dz, dgamma / dbeta / dbias, dw, every dgrad / upcat
contribution, the dy wiring -- with the walked ops and their trace keys exactly expected_walk's.  Nothing below n is looked at but
what an op from n on reads: the handed-over buffers, taken as the GPU holds them.  The bars are the existing ones, unchanged:
CONV_BAR, BN_BAR, KINK and KINK_SHARE of tests/train_kernel_ref.py; a value the BF16_ACT kernels store in bf16 adds that one
rounding, U |ref|, as tests/test_gpu_train_bf16_act.py (b16_ratio) and test_gpu_train_bf16_act_step.py hold them."""
import torch

from tests import train_kernel_ref as K
from tests import train_states as S
from yolo_v3_amd import arch

U = 2.0 ** -8                       # bf16's unit roundoff (tests/test_gpu_train_bf16_act.py)


def frozen_through(last, num_class=3):
    """The state "everything through the module `last` (in graph order) frozen and in eval mode, the rest trainable in train mode"."""
    names = [sp.name for sp in arch.conv_specs(num_class)]
    inside = set(names[:names.index(last) + 1])

    def owner(param_name):
        return param_name.rsplit(".", 2)[0] if ".conv." in param_name or ".bn." in param_name else param_name.rsplit(".", 1)[0]
    return S.State("through_" + last, lambda n: owner(n) not in inside, lambda p: (p not in inside, S.MOMENTUM, S.EPS, 0))


# everything but pre_det3.* frozen, the whole net in .eval(): pre_det3's BatchNorms train their gamma / beta on the running statistics
BUT_PRE_DET3 = S.State("all_but_pre_det3_eval", lambda n: n.startswith("pre_det3."), lambda p: (False, S.MOMENTUM, S.EPS, 0),
                       modes=lambda net: net.eval())
# prefix length -> state; and, written by hand from the graph, the buffers each hands over: (read as src / src2, read as a residual,
# prefix heads).  f14 / f23: the route tails (Darknet layers 36 / 61), f28: the backbone's output; a cut after feature.mlist.5.conv1
# leaves conv2 reading f5a and adding the block's input f4
CUTS = {52: S.STATES["backbone_eval_frozen"], 68: BUT_PRE_DET3, 8: frozen_through("feature.mlist.5.conv1")}
HANDED = {52: ({"f14", "f23", "f28"}, set(), set()),
          68: ({"f14", "up2"}, set(), {"pre_det1.logits", "pre_det2.logits"}),
          8: ({"f5a"}, {"f4"}, set())}


def b16(t):
    """int16 bf16 bits (GPU) -> float64 values (CPU), same shape."""
    return t.detach().cpu().view(torch.bfloat16).double()


def nchw(t, shape):
    """A flat or NHWC bf16 (int16) / fp32 GPU buffer of NHWC `shape` -> NCHW float64 on the CPU."""
    v = b16(t) if t.dtype == torch.int16 else t.detach().cpu().double()
    return v.reshape(shape).permute(0, 3, 1, 2)


def b16_ratio(got, ref, growth=0.0, mask=None):
    """A bf16 output: |got - ref| <= U |ref| + BN_BAR max|ref| (+ growth); `mask`: elements left out (undecided dz)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    tol = U * ref.abs() + K.BN_BAR * max(float(ref.abs().max()), 1e-30) + torch.as_tensor(growth, dtype=torch.float64)
    if mask is not None:
        got = torch.where(mask, ref, got)
    return K.ratio(got, ref, tol)


def check_from(n, net, sd, run, pg, state, what, gone=None):
    """Ops [n, 75) of the traced step `run` against float64 on the GPU's own inputs; sd: the state_dict before the step; gone: buffers
    the run no longer holds (BF16_ACT frees a bf16 buffer after its last reader), by name, as the GPU held them."""
    from tests.test_gpu_train_local import Worst
    from yolo_v3_amd import F32, BF16, BF16_ACT
    f32, bf, act = run.math == F32, run.math == BF16, run.math == BF16_ACT
    assert f32 or bf or act
    r = (lambda t: t) if f32 else K.rb                                  # the rounding of a conv operand
    ops, keys = run.ops, K.op_params(net, run.ops)
    bufs, bufs_b, tr, shape = run.bufs, run.bufs_b, run.trace, run.shape
    walk = S.expected_walk(state, ops)
    assert all(walk[i] is None for i in range(n))
    assert sorted(tr) == [i for i in range(len(ops)) if walk[i] is not None]
    assert sorted(run.saved) == list(range(n, len(ops)))
    P = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}       # parameters (unchanged) and the new running stats
    before = {k: v.detach().cpu().double() for k, v in sd.items()}
    w = Worst()
    cache = {}

    def value(name):
        """A buffer's stored value (the residual an op adds, the y it wrote): fp32 where the mode keeps one, else the bf16 plane."""
        if ("v", name) not in cache:
            if name in bufs:
                t = bufs[name]
            else:
                t = bufs_b[name] if name in bufs_b else gone[name]
            cache["v", name] = nchw(t, shape[name])
        return cache["v", name]

    def operand(name):
        """A buffer as the convs read it: the fp32 tensor (F32), else the bf16 plane."""
        if f32:
            return value(name)
        if ("o", name) not in cache:
            cache["o", name] = nchw(bufs_b[name] if name in bufs_b else gone[name], shape[name])
        return cache["o", name]

    def conv_in(op):
        return operand(op.src) if op.src2 is None else K.upcat(operand(op.src2), operand(op.src))

    if bf:                  # a buffer held both ways: the bf16 plane is bitwise the fp32 tensor rounded by torch
        for name in set(bufs) & set(bufs_b):
            assert torch.equal(bufs_b[name].view(-1), bufs[name].to(torch.bfloat16).view(torch.int16).view(-1)), name
    # ---- forward
    stats = {}
    for i in range(n, len(ops)):
        op, (kw, kb, kbn) = ops[i], keys[i]
        st = op.conv.stride[0]
        ref, sc = K.conv_fwd(conv_in(op), r(P[kw]), st, P[kb] if kb else None)
        if op.head:
            w.add("z", op.out, K.conv_ratio(nchw(bufs[op.out], shape[op.out]), ref, sc))
            continue
        sv = run.saved[i]
        assert sv["z"].dtype == (torch.int16 if act else torch.float32)
        z = nchw(sv["z"], shape[op.out])
        w.add("z", op.out, K.ratio(z, ref, (U * ref.abs() if act else 0.0) + K.CONV_BAR * sc + 1e-30))
        zr = K.rows(z)
        mean_g, invstd_g = sv["mean"].cpu().double(), sv["invstd"].cpu().double()
        training, mom, eps = state.bn(kbn)[0], state.factor(kbn), state.bn(kbn)[2]
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
        res = K.rows(value(op.res)) if op.res is not None else None
        y = K.bn_act_fwd(zr, mean_g, invstd_g, P[kbn + ".weight"], P[kbn + ".bias"], res)
        w.add("y", op.out, (b16_ratio if act else K.bn_ratio)(K.rows(value(op.out)), y))
        stats[i] = (zr, mean_g, invstd_g)
    # ---- backward, in the order the graph runs it
    consumers = {}
    for op in ops:
        for b in (op.src, op.src2, op.res):
            if b is not None and b != "x":
                consumers[b] = consumers.get(b, 0) + 1
    last, count = {}, {}
    for i, op in enumerate(ops):
        if op.head and i >= n:
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
        assert t["dy"].dtype == torch.float32 and torch.equal(t["dy"], last[op.out]), op.out       # what its consumers left, bitwise
        dy = nchw(t["dy"], shape[op.out])
        Bn, cout, Ho, Wo = dy.shape
        if act:                                                        # dz is born in bf16, in rows padded to 8 channels with zeros
            cp = (cout + 7) // 8 * 8
            assert t["dz"].dtype == torch.int16 and t["dz"].numel() == Bn * Ho * Wo * cp
            dzp = t["dz"].view(Bn, Ho, Wo, cp)
            assert not bool(dzp[..., cout:].any()), op.out
            dz_gpu = nchw(dzp[..., :cout].contiguous(), (Bn, Ho, Wo, cout))
        else:
            dz_gpu = nchw(t["dz"], shape[op.out])
        if op.head:
            if act:                                                    # dL/dloss = 1: a pure cast
                assert torch.equal(dzp[..., :cout], t["dy"].to(torch.bfloat16).view(torch.int16)), op.out
            else:                                                      # ... one exact fp32 multiply
                assert torch.equal(t["dz"], t["dy"]), op.out
            _, db, da = K.bias_bwd(K.rows(dy))
            w.add("dbias", op.out, K.ratio(t["dbias"], db, K.BN_BAR * da + 1e-30))
            assert torch.equal(pg[id(named[kb])], t["dbias"])
        else:
            zr, mean_g, invstd_g = stats[i]
            b = K.bn_act_bwd(zr, K.rows(dy), mean_g, invstd_g, P[kbn + ".weight"], P[kbn + ".bias"], state.bn(kbn)[0])
            und, total = und + int(b["und"].sum()), total + b["und"].numel()
            if act:
                w.add("dz", op.out, b16_ratio(K.rows(dz_gpu), b["dz"], b["dz_growth"], b["und"]))
                w.add("dgamma", op.out, K.bn_ratio(t["dgamma"], b["dgamma"], b["S"]))
                w.add("dbeta", op.out, K.bn_ratio(t["dbeta"], b["dbeta"], b["S"]))
            else:
                for k_, v in K.bn_bwd_ratios(K.rows(dz_gpu), t["dgamma"], t["dbeta"], b).items():
                    w.add(k_, op.out, v)
            assert torch.equal(pg[id(named[kbn + ".weight"])], t["dgamma"]) and torch.equal(pg[id(named[kbn + ".bias"])], t["dbeta"])
            if "res_after" in walk[i]:
                want = t["dy"] if "res_before" not in t else (t["res_before"].double() + t["dy"].double()).float()
                assert torch.equal(t["res_after"], want), op.out       # one fp32 add per element: exact
                contribute(op.res, t["res_after"])
        dz = r(dz_gpu)
        xin = conv_in(op)
        if "dw" in walk[i]:
            ref, sc = K.conv_wgrad(xin, P[kw].shape, dz, st)
            w.add("dw", op.out, K.conv_ratio(t["dw"], ref, sc))
            assert torch.equal(pg[id(named[kw])].view_as(t["dw"]), t["dw"])
        assert op.src != "x"                                           # (n >= 4: layer 0 is never walked)
        if not walk[i] & {"dx_after", "dcat"}:                         # no input is needed: no dgrad ran
            assert not set(t) & {"dx_after", "dcat", "dlow_after", "dtail_after"}, op.out
            continue
        ref, sc = K.conv_dgrad(xin.shape, r(P[kw]), dz, st)
        if op.cin_up == 0:
            if "dx_before" in t:
                base = nchw(t["dx_before"], shape[op.src])
                ref, sc = ref + base, sc + base.abs()
            w.add("dx" + ("+=" if "dx_before" in t else ""), op.out, K.conv_ratio(nchw(t["dx_after"], shape[op.src]), ref, sc))
            contribute(op.src, t["dx_after"])
        else:
            dcat = t["dcat"].detach().cpu().double().permute(0, 3, 1, 2)
            w.add("dcat", op.out, K.conv_ratio(dcat, ref, sc))
            rl, sl, rt = K.upcat_bwd(dcat, op.cin_up)
            if "dlow_before" in t:
                base = nchw(t["dlow_before"], shape[op.src2])
                rl, sl = rl + base, sl + base.abs()
            if "dlow_after" in walk[i]:
                w.add("dlow", op.out, K.ratio(nchw(t["dlow_after"], shape[op.src2]), rl, K.BN_BAR * sl + 1e-30))
                contribute(op.src2, t["dlow_after"])
            if "dtail_after" in walk[i]:
                if "dtail_before" in t:
                    rt = (nchw(t["dtail_before"], shape[op.src]) + rt).float().double()
                assert torch.equal(nchw(t["dtail_after"], shape[op.src]), rt), op.out      # a copy or one fp32 add: exact
                contribute(op.src, t["dtail_after"])
    assert set(pg) == want_pg                                          # exactly the gradients of the walked ops' parameters
    share = und / max(total, 1)
    print("%s: %d of %d BN elements undecided at the kink (%.3g)" % (what, und, total, share))
    assert share <= K.KINK_SHARE
    w.report(what)
