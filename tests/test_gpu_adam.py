"""yolo_v3_amd.optim.Adam / AdamW on the GPU: step and step_clipped bit for bit against the numpy definition (tests/adam_ref.py) at
the chunk edges, across kernel-argument blocks, at 4-byte alignment, with skipped gradients, under every setting and with draws
that reach the subnormals; against torch within the float64 bar of test_adam_host.py; and through three training steps of the
80-class net."""
import copy

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import frozen_prefix_check as FC
from tests import optim_ref as R
from tests import test_gpu_train_bf16 as GB
from tests import test_gpu_train_local as L
from tests import yolo_loss_ref as YR
from tests.test_gpu_optim import DEV, draws, host, norm_bits, on_gpu
from yolo_v3_amd import BF16, arch, backprop, optim

pytestmark = pytest.mark.gpu
CH = optim.CHUNK
EDGES = [1, 3, CH - 1, CH, CH + 1, 2 * CH + 5]
STATE = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def ref_kwargs(group):
    """A param group's hyper-parameters under tests/adam_ref.py's keyword names."""
    return dict(lr=float(group["lr"]), betas=group["betas"], eps=group["eps"], weight_decay=group["weight_decay"],
                amsgrad=group["amsgrad"], maximize=group["maximize"], decoupled=group["decoupled_weight_decay"])


CLASSES = {"Adam": (optim.Adam, torch.optim.Adam), "AdamW": (optim.AdamW, torch.optim.AdamW)}


def ctor(h, which):
    """((our class, torch's), torch's keywords) of one of adam_ref.SETTINGS under class `which`.  AdamW runs every setting with
    decoupled decay (the setting's weight_decay, or its own default 1e-2 where the setting has none); Adam runs them as they are,
    the decoupled one through decoupled_weight_decay=True."""
    h = dict(h)
    decoupled = h.pop("decoupled", False)
    if which == "Adam" and decoupled:
        h["decoupled_weight_decay"] = True
    return CLASSES[which], h


class Beside:
    """An optim.Adam / AdamW over fresh GPU parameters beside the numpy model of the same optimizer."""

    def __init__(self, arrays, cls=optim.Adam, groups=None, p_off=None, **hyper):
        n = len(arrays)
        p_off = p_off or [0] * n
        self.params = [torch.nn.Parameter(on_gpu(a, o)) for a, o in zip(arrays, p_off)]
        self.p = [a.copy() for a in arrays]
        self.m, self.v, self.x, self.t = [None] * n, [None] * n, [None] * n, [0] * n
        groups = groups or [dict(idx=list(range(n)))]
        self.idx = [g["idx"] for g in groups]
        self.opt = cls([dict({k: v for k, v in g.items() if k != "idx"}, params=[self.params[i] for i in g["idx"]])
                        for g in groups], **hyper)

    def give(self, grads, g_off=None):
        """Fresh .grad tensors (None: no gradient)."""
        self.g = grads
        for i, (p, g) in enumerate(zip(self.params, grads)):
            p.grad = None if g is None else on_gpu(g, (g_off or {}).get(i, 0)).view(p.shape)

    def live(self):
        return [i for ix in self.idx for i in ix if self.g[i] is not None and self.params[i].requires_grad]

    def ref_norm(self, max_norm):
        return R.norm_and_coef([self.g[i] for i in self.live()], max_norm)

    def ref_step(self, max_norm=None):
        """The numpy model's step with the hyper-parameters the optimizer's param_groups hold now; returns (total_norm, coef)."""
        norm, coef = self.ref_norm(max_norm) if max_norm is not None else (None, None)
        for ix, grp in zip(self.idx, self.opt.param_groups):
            for i in ix:
                if self.g[i] is None or not self.params[i].requires_grad:
                    continue
                self.t[i] += 1
                self.p[i], self.m[i], self.v[i], self.x[i] = A.adam(self.p[i], self.g[i], self.m[i], self.v[i], self.x[i], self.t[i],
                                                                    coef=coef, **ref_kwargs(grp))
        return norm, coef

    def check(self, what=""):
        torch.cuda.synchronize()
        for i, p in enumerate(self.params):
            assert R.same_bits(host(p), self.p[i]), "%s: parameter %d (%d elements)" % (what, i, p.numel())
            st = self.opt.state.get(p) or {}
            assert bool(st) == (self.t[i] > 0), "%s: state of parameter %d" % (what, i)
            if not st:
                continue
            step = st["step"]
            assert step.device.type == "cpu" and step.dtype == torch.float32 and step.dim() == 0 and float(step) == self.t[i], (what, i)
            for key, want in zip(STATE, (self.m[i], self.v[i], self.x[i])):
                assert (key in st) == (want is not None), "%s: %s of parameter %d" % (what, key, i)
                assert want is None or R.same_bits(host(st[key]), want), "%s: %s of parameter %d" % (what, key, i)


def clipped_steps(b, sizes, seed, max_norm, g_off=None, skip=lambda k: (), steps=3, scale=1.0):
    for k in range(steps):
        grads = draws(sizes, seed + k, scale)
        b.give([None if i in skip(k) else g for i, g in enumerate(grads)], g_off)
        versions = [p._version for p in b.params]
        norm = b.opt.step_clipped(max_norm)
        want, coef = b.ref_step(max_norm)
        assert norm_bits(norm, want), (k, float(norm), float(want))
        b.check("step %d" % k)
        for i, p in enumerate(b.params):
            assert (p._version > versions[i]) == (i in b.live()), i
    return coef


AMS = dict(lr=0.01, weight_decay=5e-4, amsgrad=True)


# ---------------------------------------------------------------- geometry
def test_chunk_edges():
    b = Beside(draws(EDGES, 1, 0.1), **AMS)
    coef = clipped_steps(b, EDGES, 10, 5.0)
    assert 0 < coef < 1


def test_more_tensors_than_one_kernel_argument_block():
    sizes = [1] * 300
    b = Beside(draws(sizes, 2, 0.1), **AMS)
    coef = clipped_steps(b, sizes, 20, 3.0)
    assert 0 < coef < 1


@pytest.mark.parametrize("which", ["param", "grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"])
def test_four_byte_aligned_views_take_the_scalar_path(which):
    """A parameter / gradient / state tensor that is storage[1:], beside an aligned partner of the same size."""
    sizes = [CH + 7, CH + 7, 5]
    b = Beside(draws(sizes, 3, 0.1), p_off=[1 if which == "param" else 0, 0, 0], **AMS)
    g_off = {0: 1} if which == "grad" else None
    p0 = b.params[0]
    if which in STATE:
        b.give(draws(sizes, 29))
        b.opt.step()
        b.ref_step()
        b.opt.state[p0][which] = on_gpu(host(b.opt.state[p0][which]), 1)
    assert (p0.data_ptr() % 16 != 0) == (which == "param") and b.params[1].data_ptr() % 16 == 0
    clipped_steps(b, sizes, 30, 5.0, g_off)
    if which == "grad":
        assert p0.grad.data_ptr() % 16 == 4
    for key in STATE:
        assert b.opt.state[p0][key].data_ptr() % 16 == (4 if key == which else 0)


def test_a_skipped_gradient_leaves_the_parameter_and_its_step_lags():
    sizes = [CH + 1, 100, 7, 2 * CH, 33]
    arrays = draws(sizes, 4, 0.1)
    b = Beside(arrays, **AMS)
    b.params[3].requires_grad_(False)                               # has a .grad, is never stepped
    clipped_steps(b, sizes, 40, 5.0, skip=lambda k: {1} if k == 1 else ())
    assert b.t == [3, 2, 3, 0, 3]                                   # 1 was stepped on steps 1 and 3 with bias corrections of 1 and 2
    assert float(b.opt.state[b.params[1]]["step"]) == 2 and float(b.opt.state[b.params[0]]["step"]) == 3
    assert R.same_bits(host(b.params[3]), arrays[3]) and not b.opt.state.get(b.params[3])


# ---------------------------------------------------------------- settings
SIZES = [CH + 9, 77, 1]


@pytest.mark.parametrize("name", sorted(A.SETTINGS))
@pytest.mark.parametrize("which", sorted(CLASSES))
@pytest.mark.parametrize("clip", ["none", "clipped", "separate"])
def test_settings_first_to_third_step(name, which, clip):
    (cls, _), h = ctor(A.SETTINGS[name], which)
    b = Beside(draws(SIZES, 5, 0.1), cls, **h)
    group = b.opt.param_groups[0]
    assert group["decoupled_weight_decay"] == (which == "AdamW" or name == "decoupled")
    assert which != "AdamW" or group["weight_decay"] != 0          # AdamW: amsgrad, maximize, both lerp branches all with its decay
    for k in range(3):                                              # step 0 creates the state, steps 1 and 2 read it
        b.give(draws(SIZES, 50 + k))
        if clip == "none":
            b.opt.step()
            b.ref_step()
        elif clip == "clipped":
            norm = b.opt.step_clipped(4.0)
            assert norm_bits(norm, b.ref_step(4.0)[0])
        else:
            optim.clip_grad_norm_(b.params, 4.0)
            _, coef = b.ref_norm(4.0)
            b.g = [R.scale(g, coef) for g in b.g]
            b.opt.step()
            b.ref_step()
        b.check("%s %s step %d" % (which, name, k))


def test_two_groups_and_a_learning_rate_that_moves():
    sizes = [CH + 3, 50, 2 * CH, 9]
    groups = [dict(idx=[0, 1], lr=0.02), dict(idx=[2, 3], lr=0.002, weight_decay=0.0)]
    b = Beside(draws(sizes, 6, 0.1), optim.AdamW, groups, lr=0.5, weight_decay=1e-2)
    sched = torch.optim.lr_scheduler.StepLR(b.opt, step_size=1, gamma=0.3)
    seen = []
    for k in range(4):
        b.give(draws(sizes, 60 + k))
        if k == 3:
            b.opt.param_groups[1]["lr"] = 0.123                     # by hand
        seen.append(tuple(g["lr"] for g in b.opt.param_groups))
        b.opt.step_clipped(6.0)
        b.ref_step(6.0)
        b.check("step %d" % k)
        sched.step()
    assert seen[0] == (0.02, 0.002) and seen[1][0] == pytest.approx(0.006) and seen[3][1] == 0.123 and len(set(seen)) == 4


# ---------------------------------------------------------------- the clip coefficient
def test_clip_coefficient_below_one_at_one_and_not_finite():
    sizes = [CH + 5, 31]
    grads = draws(sizes, 70)
    for max_norm, kind in ((2.0, "below"), (1e6, "one")):
        b = Beside(draws(sizes, 7, 0.1), **AMS)
        b.give(grads)
        norm = b.opt.step_clipped(max_norm)
        want, coef = b.ref_step(max_norm)
        assert norm_bits(norm, want) and ((0 < coef < 1) if kind == "below" else coef == 1)
        b.check(kind)
    for bad in (np.inf, np.nan):                                    # nothing raises; the bits are the definition's, NaNs included
        c = Beside(draws(sizes, 7, 0.1), **AMS)
        spoiled = [g.copy() for g in grads]
        spoiled[0][CH + 1] = bad
        for k in range(2):                                          # the second step reads the NaNs the first left in the state
            c.give(spoiled if k == 0 else grads)
            norm = c.opt.step_clipped(2.0)
            want, coef = c.ref_step(2.0)
            assert norm_bits(norm, want)
            c.check("non-finite, step %d" % k)
        assert np.isnan(c.p[0]).sum() == (1 if np.isinf(bad) else sizes[0]) and np.isnan(c.x[0]).sum() == np.isnan(c.p[0]).sum()


def test_step_clipped_is_clip_then_step_and_leaves_the_gradients():
    sizes = EDGES + [40]
    a, b = Beside(draws(sizes, 8, 0.1), **AMS), Beside(draws(sizes, 8, 0.1), **AMS)
    for k in range(2):
        grads = draws(sizes, 80 + k)
        a.give(grads)
        b.give(grads)
        na = a.opt.step_clipped(5.0).clone()
        nb = optim.clip_grad_norm_(b.params, 5.0).clone()
        b.opt.step()
        torch.cuda.synchronize()
        assert torch.equal(na, nb) and float(na) > 5.0
        for pa, pb, g in zip(a.params, b.params, grads):
            assert torch.equal(pa, pb) and all(torch.equal(a.opt.state[pa][key], b.opt.state[pb][key]) for key in STATE)
            assert R.same_bits(host(pa.grad), g) and not R.same_bits(host(pb.grad), g)


def test_repeated_runs_give_identical_bits():
    sizes = EDGES + [5 * CH + 11]
    runs = []
    for _ in range(2):
        b = Beside(draws(sizes, 9, 0.1), **AMS)
        out = []
        for k in range(2):
            b.give(draws(sizes, 90 + k))
            out.append(host(b.opt.step_clipped(5.0)).copy())
        torch.cuda.synchronize()
        out += [host(p).copy() for p in b.params] + [host(b.opt.state[p][key]).copy() for p in b.params for key in STATE]
        runs.append(out)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*runs))


@pytest.mark.parametrize("eps", [1e-8, 0.0])
@pytest.mark.parametrize("which", sorted(CLASSES))
@pytest.mark.parametrize("name", ["default", "beta1_04", "decoupled", "maximize"])        # (no L2 decay: it would lift g off the subnormals)
def test_draws_that_reach_the_subnormals(name, which, eps):
    """|g| from 1e-22 to 1e2 and exact zeros: g * g is subnormal or 0 for many elements, sqrt and the divisions see subnormals and
    (with eps = 0) 0 / 0.  Correctly rounded sqrt and divide with denormals kept are what make these bits the definition's."""
    (cls, _), h = ctor(dict(A.SETTINGS[name], eps=eps), which)
    sizes = [CH + 9, 77]
    b = Beside(draws(sizes, 11, 0.1), cls, **h)
    for k in range(3):
        b.give([A.wide_draws(n, 110 + 2 * k + j) for j, n in enumerate(sizes)])
        b.opt.step() if k else b.opt.step_clipped(1e-3)
        b.ref_step(None if k else 1e-3)
        b.check("step %d" % k)
    v = b.v[0]
    assert np.any((v > 0) & (v < 1.17e-38)) and (eps != 0 or np.isnan(b.p[0]).any())


# ---------------------------------------------------------------- against torch
@pytest.mark.parametrize("which", sorted(CLASSES))
@pytest.mark.parametrize("name", ["default", "l2", "decoupled", "amsgrad", "beta1_04", "maximize"])
def test_against_torch_on_the_gpu_within_the_float64_bar(name, which):
    (ours, theirs), h = ctor(A.SETTINGS[name], which)
    sizes = [CH + 9, 77]
    arrays, ms, grads = draws(sizes, 11, 0.1), draws(sizes, 12, 0.3), draws(sizes, 13)
    vs = [np.square(x) for x in draws(sizes, 14, 0.5)]
    xs = [np.square(x) for x in draws(sizes, 15, 0.5)]
    sides = {}
    for cls in (ours, theirs):
        params = [torch.nn.Parameter(on_gpu(a)) for a in arrays]
        opt = cls(params, foreach=False, **h)
        for p, m, v, x, g in zip(params, ms, vs, xs, grads):
            opt.state[p]["step"] = torch.tensor(4.0)
            opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"] = on_gpu(m), on_gpu(v)
            if h.get("amsgrad"):
                opt.state[p]["max_exp_avg_sq"] = on_gpu(x)
            p.grad = on_gpu(g)
        opt.step()
        torch.cuda.synchronize()
        assert all(float(opt.state[p]["step"]) == 5 for p in params)
        sides[cls] = [[host(p)] + [host(opt.state[p][key]) if key in opt.state[p] else None for key in STATE] for p in params]
    group = ours([torch.nn.Parameter(torch.zeros(1))], **h).param_groups[0]
    for i in range(len(sizes)):
        x0 = xs[i] if h.get("amsgrad") else None
        p64, m64, v64, _, scales = A.adam64(arrays[i], grads[i], ms[i], vs[i], x0, 5, **ref_kwargs(group))
        for cls, side in sides.items():
            ratios = A.bar_ratios(side[i][:3], (p64, m64, v64), scales)
            assert max(ratios) <= A.K, (cls.__name__, i, ratios)
        want = A.adam(arrays[i], grads[i], ms[i], vs[i], x0, 5, **ref_kwargs(group))
        assert all(w is None or R.same_bits(s, w) for s, w in zip(sides[ours][i], want)), i


@pytest.mark.parametrize("name,which", [("amsgrad", "Adam"), ("amsgrad", "AdamW"), ("decoupled", "Adam"), ("maximize", "AdamW")])
def test_state_dict_round_trip_with_torch(name, which):
    (ours, theirs), h = ctor(A.SETTINGS[name], which)
    sizes = [CH + 9, 77, 3]
    b = Beside(draws(sizes, 14, 0.1), ours, **h)
    kw = ref_kwargs(b.opt.param_groups[0])
    t_params = [torch.nn.Parameter(on_gpu(a)) for a in b.p]
    t_opt = theirs(t_params, foreach=False, **h)
    g0, g1, g2 = draws(sizes, 140), draws(sizes, 141), draws(sizes, 142)
    b.give(g0)
    b.opt.step()
    b.ref_step()
    # ours -> torch: torch continues from our state within the bar
    t_opt.load_state_dict(copy.deepcopy(b.opt.state_dict()))       # (load_state_dict keeps the tensors it is given: a copy each)
    with torch.no_grad():
        for tp, p in zip(t_params, b.params):
            tp.copy_(p)
    before = [[x.copy() if x is not None else None for x in (b.p[i], b.m[i], b.v[i], b.x[i])] for i in range(len(sizes))]
    for tp, g in zip(t_params, g1):
        tp.grad = on_gpu(g)
    t_opt.step()
    b.give(g1)
    b.opt.step()
    b.ref_step()
    b.check("after our own second step")
    for i, tp in enumerate(t_params):
        st = t_opt.state[tp]
        assert float(st["step"]) == 2 and st["step"].device.type == "cpu"
        p0, m0, v0, x0 = before[i]
        p64, m64, v64, _, scales = A.adam64(p0, g1[i], m0, v0, x0, 2, **kw)
        ratios = A.bar_ratios((host(tp), host(st["exp_avg"]), host(st["exp_avg_sq"])), (p64, m64, v64), scales)
        assert max(ratios) <= A.K, (i, ratios)
    # torch -> ours: we continue from torch's state, bitwise to the definition on that state
    c = Beside([host(tp) for tp in t_params], ours, **h)
    c.opt.load_state_dict(copy.deepcopy(t_opt.state_dict()))
    for i, tp in enumerate(t_params):
        st = t_opt.state[tp]
        c.m[i], c.v[i], c.t[i] = host(st["exp_avg"]).copy(), host(st["exp_avg_sq"]).copy(), 2
        c.x[i] = host(st["max_exp_avg_sq"]).copy() if "max_exp_avg_sq" in st else None
    c.give(g2)
    c.opt.step_clipped(5.0)
    c.ref_step(5.0)
    c.check("continued from torch's state")


def test_a_fused_group_and_torchs_fused_checkpoint_resume_with_step_on_the_cpu():
    """load_state_dict moves `step` to the parameter's device when the group says fused=True, and torch's fused Adam keeps it there:
    both come back to the CPU at the load, and the next step is the definition's on the loaded state."""
    sizes, h = [CH + 9, 77], dict(lr=0.01, weight_decay=1e-2, amsgrad=True)
    b = Beside(draws(sizes, 16, 0.1), optim.AdamW, fused=True, **h)
    b.give(draws(sizes, 160))
    b.opt.step()
    b.ref_step()
    c = Beside([x.copy() for x in b.p], optim.AdamW, fused=True, **h)          # a resume from our own checkpoint
    c.opt.load_state_dict(copy.deepcopy(b.opt.state_dict()))
    c.m, c.v, c.x, c.t = [x.copy() for x in b.m], [x.copy() for x in b.v], [x.copy() for x in b.x], list(b.t)
    c.give(draws(sizes, 161))
    c.opt.step_clipped(5.0)
    c.ref_step(5.0)
    c.check("resumed under fused=True")
    t_params = [torch.nn.Parameter(on_gpu(a)) for a in b.p]                     # a checkpoint of torch's fused AdamW
    t_opt = torch.optim.AdamW(t_params, fused=True, **h)
    for tp, g in zip(t_params, draws(sizes, 162)):
        tp.grad = on_gpu(g)
    t_opt.step()
    torch.cuda.synchronize()
    assert all(t_opt.state[tp]["step"].is_cuda for tp in t_params)
    d = Beside([host(tp) for tp in t_params], optim.AdamW, **h)
    d.opt.load_state_dict(copy.deepcopy(t_opt.state_dict()))
    for i, tp in enumerate(t_params):
        st = t_opt.state[tp]
        d.m[i], d.v[i], d.x[i], d.t[i] = host(st["exp_avg"]).copy(), host(st["exp_avg_sq"]).copy(), host(st["max_exp_avg_sq"]).copy(), 1
    d.give(draws(sizes, 163))
    d.opt.step_clipped(5.0)
    d.ref_step(5.0)
    d.check("continued from torch's fused state")


# ---------------------------------------------------------------- the whole net
def test_three_training_steps_of_the_80_class_net():
    hw, nc, B = (96, 96), 80, 2
    net = L.make_net(hw, nc, BF16).train()
    backbone = {id(p) for p in net.feature.parameters()}
    opt = optim.AdamW([{"params": [p for p in net.parameters() if id(p) not in backbone], "lr": 1e-3},
                       {"params": list(net.feature.parameters()), "lr": 1e-4}], 1e-3, weight_decay=5e-4)
    names = {id(p): k for k, p in net.named_parameters()}
    order = [[names[id(p)] for p in g["params"]] for g in opt.param_groups]
    assert [len(o) for o in order] == [66, 156]
    named = dict(net.named_parameters())
    ref = {k: (host(p).copy(), None, None, None) for k, p in named.items()}
    x = L.images(B, hw, 31)
    tg = YR.random_rows(77, B, 8, nc, (0.05, 0.7))
    for k in range(3):
        GB.gpu_step(net, x, tg)
        grads = {key: host(p.grad).copy() for key, p in named.items()}
        versions = {key: p._version for key, p in named.items()}
        norm = opt.step_clipped(1000.0)
        want, coef = R.norm_and_coef([grads[key] for o in order for key in o], 1000.0)
        assert norm_bits(norm, want), (k, float(norm), float(want))
        for o, grp in zip(order, opt.param_groups):
            for key in o:
                ref[key] = A.adam(ref[key][0], grads[key], ref[key][1], ref[key][2], ref[key][3], k + 1, coef=coef, **ref_kwargs(grp))
        for key, p in named.items():
            st = opt.state[p]
            assert R.same_bits(host(p), ref[key][0]), (k, key)
            assert R.same_bits(host(st["exp_avg"]), ref[key][1]) and R.same_bits(host(st["exp_avg_sq"]), ref[key][2]), (k, key)
            assert float(st["step"]) == k + 1 and "max_exp_avg_sq" not in st
            assert p._version > versions[key], (k, key)
            assert R.same_bits(host(p.grad), grads[key]), (k, key)


def test_a_step_on_the_heads_leaves_the_frozen_prefix_engine_packed():
    n, hw, nc = 52, (96, 96), 3
    net = FC.CUTS[n].apply(L.make_net(hw, nc, BF16))
    net.frozen_prefix = True
    trainable = [p for p in net.parameters() if p.requires_grad]
    opt = optim.Adam(trainable, lr=1e-3)
    x, tg = L.images(2, hw, 31), YR.random_rows(108, 2, 8, nc, (0.05, 0.7))
    l0 = float(GB.gpu_step(net, x, tg).detach())
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt.step_clipped(1000.0)
    l1 = float(GB.gpu_step(net, x, tg).detach())
    opt.step_clipped(1000.0)
    torch.cuda.synchronize()
    eng = net.prefix_engine(backprop.PREFIX_MODE[BF16], n)
    assert list(net._prefix_engines) == [(backprop.PREFIX_MODE[BF16], n)] and eng.generation == 1
    moved = {k for k, v in net.state_dict().items() if not torch.equal(v, before[k])}
    prefix = tuple(sp.name + "." for sp in arch.conv_specs(nc)[:n])
    assert moved and not any(k.startswith(prefix) for k in moved)
    assert l1 != l0


# ---------------------------------------------------------------- errors
def test_a_bad_state_tensor_raises_type_error_and_no_parameter_changes():
    sizes = [64, 64]
    b = Beside(draws(sizes, 15), **AMS)
    b.give(draws(sizes, 150))
    b.opt.step()
    b.ref_step()
    b.check("first step")
    good = b.opt.state[b.params[1]]
    kept = dict(good)
    for key, bad in (("exp_avg", good["exp_avg"].double()), ("exp_avg_sq", good["exp_avg_sq"].cpu()),
                     ("max_exp_avg_sq", good["max_exp_avg_sq"][:32]), ("exp_avg", good["exp_avg"].view(8, 8).t()),
                     ("step", good["step"].to(DEV))):
        good[key] = bad
        for call in (b.opt.step, lambda: b.opt.step_clipped(1.0)):
            with pytest.raises(TypeError):
                call()
        good[key] = kept[key]
    del good["max_exp_avg_sq"]
    with pytest.raises(TypeError):
        b.opt.step()
    good["max_exp_avg_sq"] = kept["max_exp_avg_sq"]
    with pytest.raises(ValueError):
        optim.Adam([torch.nn.Parameter(on_gpu(draws([4], 1)[0]))], lr=torch.tensor(0.1, device=DEV))
    b.check("after the refusals")                                   # parameter 0 came before the bad one: it was not stepped either
    b.give(draws(sizes, 151))
    b.opt.step()
    b.ref_step()
    b.check("and the optimizer still works")
