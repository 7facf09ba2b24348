"""yolo_v3_amd.optim on the GPU: clip_grad_norm_, SGD.step and SGD.step_clipped bit for bit against the numpy definition
(tests/optim_ref.py) at the chunk edges, across kernel-argument blocks, at 4-byte alignment, with sparse gradients and under every
setting; against torch within the float64 bar of test_optim_host.py; and through three training steps of the 80-class net."""
import copy

import numpy as np
import pytest
import torch

from tests import frozen_prefix_check as FC
from tests import optim_ref as R
from tests import test_gpu_train_bf16 as GB
from tests import test_gpu_train_local as L
from tests import yolo_loss_ref as YR
from yolo_v3_amd import BF16, arch, backprop, optim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = optim.CHUNK
EDGES = [1, 3, CH - 1, CH, CH + 1, 2 * CH + 5]
MOM = dict(lr=0.01, momentum=0.9, weight_decay=5e-4)


def on_gpu(a, off=0):
    """The fp32 array on the GPU, `off` elements into its storage (off = 1: 4-byte aligned only)."""
    st = torch.empty(a.size + off, device=DEV, dtype=torch.float32)
    v = st[off:]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return v


def host(t):
    return t.detach().cpu().numpy()


def draws(sizes, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * scale).astype(np.float32) for n in sizes]


class Beside:
    """An optim.SGD over fresh GPU parameters beside the numpy model of the same optimizer."""

    def __init__(self, arrays, groups=None, p_off=None, **hyper):
        n = len(arrays)
        p_off = p_off or [0] * n
        self.params = [torch.nn.Parameter(on_gpu(a, o)) for a, o in zip(arrays, p_off)]
        self.p = [a.copy() for a in arrays]
        self.buf = [None] * n
        groups = groups or [dict(idx=list(range(n)))]
        self.idx = [g["idx"] for g in groups]
        self.opt = optim.SGD([dict({k: v for k, v in g.items() if k != "idx"}, params=[self.params[i] for i in g["idx"]])
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
                self.p[i], self.buf[i] = R.sgd(self.p[i], self.g[i], self.buf[i], grp["lr"], grp["momentum"], grp["dampening"],
                                               grp["weight_decay"], grp["nesterov"], grp["maximize"], coef)
        return norm, coef

    def check(self, what=""):
        torch.cuda.synchronize()
        for i, p in enumerate(self.params):
            assert R.same_bits(host(p), self.p[i]), "%s: parameter %d (%d elements)" % (what, i, p.numel())
            buf = self.opt.state[p].get("momentum_buffer") if p in self.opt.state else None
            assert (buf is None) == (self.buf[i] is None), "%s: state of parameter %d" % (what, i)
            assert buf is None or R.same_bits(host(buf), self.buf[i]), "%s: buffer %d" % (what, i)


def norm_bits(t, want):
    assert t.dtype == torch.float32 and t.dim() == 0 and t.is_cuda
    return R.same_bits(host(t).reshape(1), np.array([want], dtype=np.float32))


def three_clipped_steps(b, sizes, seed, max_norm, g_off=None, skip=()):
    for k in range(3):
        grads = draws(sizes, seed + k)
        b.give([None if i in skip else g for i, g in enumerate(grads)], g_off)
        versions = [p._version for p in b.params]
        norm = b.opt.step_clipped(max_norm)
        want, coef = b.ref_step(max_norm)
        assert norm_bits(norm, want), (k, float(norm), float(want))
        b.check("step %d" % k)
        for i, p in enumerate(b.params):
            assert (p._version > versions[i]) == (i in b.live()), i
    return coef


# ---------------------------------------------------------------- geometry
def test_chunk_edges():
    b = Beside(draws(EDGES, 1, 0.1), **MOM)
    coef = three_clipped_steps(b, EDGES, 10, 5.0)
    assert 0 < coef < 1


def test_more_tensors_than_one_kernel_argument_block():
    sizes = [1] * 300
    b = Beside(draws(sizes, 2, 0.1), **MOM)
    coef = three_clipped_steps(b, sizes, 20, 3.0)
    assert 0 < coef < 1


@pytest.mark.parametrize("which", ["param", "grad", "both", "buffer"])
def test_four_byte_aligned_views_take_the_scalar_path(which):
    """A parameter / gradient / momentum buffer that is storage[1:], beside an aligned partner of the same size."""
    sizes = [CH + 7, CH + 7, 5]
    b = Beside(draws(sizes, 3, 0.1), p_off=[1 if which in ("param", "both") else 0, 0, 0], **MOM)
    g_off = {0: 1} if which in ("grad", "both") else None
    if which == "buffer":
        first = draws(sizes, 29)
        b.give(first)
        b.opt.step()
        b.ref_step()
        p0 = b.params[0]
        b.opt.state[p0]["momentum_buffer"] = on_gpu(host(b.opt.state[p0]["momentum_buffer"]), 1)
    assert (b.params[0].data_ptr() % 16 != 0) == (which in ("param", "both")) and b.params[1].data_ptr() % 16 == 0
    three_clipped_steps(b, sizes, 30, 5.0, g_off)
    if which in ("grad", "both"):
        assert b.params[0].grad.data_ptr() % 16 == 4
    if which == "buffer":
        assert b.opt.state[b.params[0]]["momentum_buffer"].data_ptr() % 16 == 4


def test_tensors_without_a_gradient_are_left_alone():
    sizes = [CH + 1, 100, 7, 2 * CH, 33]
    arrays = draws(sizes, 4, 0.1)
    b = Beside(arrays, **MOM)
    b.params[3].requires_grad_(False)
    three_clipped_steps(b, sizes, 40, 5.0, skip={1})                # 1: .grad is None; 3: has a .grad, requires_grad False
    for i in (1, 3):
        assert R.same_bits(host(b.params[i]), arrays[i]) and not b.opt.state.get(b.params[i])
    total = optim.clip_grad_norm_(b.params, 1e9)
    assert norm_bits(total, b.ref_norm(1e9)[0])


# ---------------------------------------------------------------- settings
SETTINGS = {
    "momentum0": dict(lr=0.01, momentum=0.0, weight_decay=5e-4),
    "momentum0_wd0": dict(lr=0.01),
    "momentum": dict(lr=0.01, momentum=0.9, weight_decay=5e-4),
    "wd0": dict(lr=0.01, momentum=0.9, weight_decay=0.0),
    "dampening": dict(lr=0.01, momentum=0.9, dampening=0.1, weight_decay=5e-4),
    "nesterov": dict(lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4),
    "maximize": dict(lr=0.01, momentum=0.9, maximize=True, weight_decay=5e-4),
    "nesterov_maximize_wd0": dict(lr=0.003, momentum=0.8, nesterov=True, maximize=True),
}
SIZES = [CH + 9, 77, 1]


@pytest.mark.parametrize("name", sorted(SETTINGS))
@pytest.mark.parametrize("clip", ["none", "clipped", "separate"])
def test_settings_first_to_third_step(name, clip):
    b = Beside(draws(SIZES, 5, 0.1), **SETTINGS[name])
    for k in range(3):                                              # step 0 creates the buffers, steps 1 and 2 read them
        b.give(draws(SIZES, 50 + k))
        if clip == "none":
            b.opt.step()
            b.ref_step()
        elif clip == "clipped":
            norm = b.opt.step_clipped(4.0)
            assert norm_bits(norm, b.ref_step(4.0)[0])
        else:
            norm = optim.clip_grad_norm_(b.params, 4.0)
            want, coef = b.ref_norm(4.0)
            assert norm_bits(norm, want)
            torch.cuda.synchronize()
            b.g = [R.scale(g, coef) for g in b.g]
            assert all(R.same_bits(host(p.grad), g) for p, g in zip(b.params, b.g))
            b.opt.step()
            b.ref_step()
        b.check("%s step %d" % (name, k))
    if not SETTINGS[name].get("momentum"):
        assert all(not b.opt.state.get(p) for p in b.params)


def test_two_groups_and_a_learning_rate_that_moves():
    sizes = [CH + 3, 50, 2 * CH, 9]
    groups = [dict(idx=[0, 1], lr=0.02), dict(idx=[2, 3], lr=0.002, weight_decay=0.0)]
    b = Beside(draws(sizes, 6, 0.1), groups, lr=0.5, momentum=0.9, weight_decay=5e-4)
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
    b = Beside(draws(sizes, 7, 0.1), **MOM)
    grads = draws(sizes, 70)
    b.give(grads)
    norm = optim.clip_grad_norm_(b.params, 2.0)                     # coef < 1
    want, coef = b.ref_norm(2.0)
    assert 0 < coef < 1 and norm_bits(norm, want)
    assert all(R.same_bits(host(p.grad), R.scale(g, coef)) for p, g in zip(b.params, grads))
    b.give(grads)
    versions = [p.grad._version for p in b.params]
    norm = optim.clip_grad_norm_(b.params, 1e6)                     # coef == 1: the gradients keep their bits
    want, coef = b.ref_norm(1e6)
    assert coef == 1 and norm_bits(norm, want)
    assert all(R.same_bits(host(p.grad), g) for p, g in zip(b.params, grads))
    assert all(p.grad._version > v for p, v in zip(b.params, versions))
    for bad in (np.inf, np.nan):                                    # nothing raises; the bits are the definition's, NaNs included
        for fused in (False, True):
            c = Beside(draws(sizes, 7, 0.1), **MOM)
            spoiled = [g.copy() for g in grads]
            spoiled[0][CH + 1] = bad
            c.give(spoiled)
            if fused:
                norm = c.opt.step_clipped(2.0)
                want, coef = c.ref_step(2.0)
            else:
                norm = optim.clip_grad_norm_(c.params, 2.0)
                want, coef = c.ref_norm(2.0)
                assert all(R.same_bits(host(p.grad), R.scale(g, coef)) for p, g in zip(c.params, spoiled))
                c.g = [R.scale(g, coef) for g in spoiled]
                c.opt.step()
                c.ref_step()
            assert norm_bits(norm, want) and (np.isnan(coef) if np.isnan(bad) else coef == 0)
            c.check("non-finite")
            assert np.isnan(c.p[0]).sum() == (1 if np.isinf(bad) else sizes[0])


def test_step_clipped_is_clip_then_step_and_leaves_the_gradients():
    sizes = EDGES + [40]
    a, b = Beside(draws(sizes, 8, 0.1), **MOM), Beside(draws(sizes, 8, 0.1), **MOM)
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
            assert torch.equal(pa, pb) and torch.equal(a.opt.state[pa]["momentum_buffer"], b.opt.state[pb]["momentum_buffer"])
            assert R.same_bits(host(pa.grad), g) and not R.same_bits(host(pb.grad), g)


def test_repeated_runs_give_identical_bits():
    sizes = EDGES + [5 * CH + 11]
    runs = []
    for _ in range(2):
        b = Beside(draws(sizes, 9, 0.1), **MOM)
        norms = []
        for k in range(2):
            b.give(draws(sizes, 90 + k))
            norms.append(host(b.opt.step_clipped(5.0)).copy())
        torch.cuda.synchronize()
        runs.append((norms, [host(p).copy() for p in b.params], [host(b.opt.state[p]["momentum_buffer"]).copy() for p in b.params]))
    (n0, p0, b0), (n1, p1, b1) = runs
    assert all(x.tobytes() == y.tobytes() for x, y in zip(n0 + p0 + b0, n1 + p1 + b1))
    g = draws(sizes, 91)
    assert n0[1] == R.norm_and_coef(g, 5.0)[0]                      # the host test's definition: fp32(sqrt(float64 sum))
    exact = np.sqrt(sum(float(np.sum(np.square(x.astype(np.float64)))) for x in g))
    assert abs(float(n0[1]) - exact) <= float(np.spacing(np.float32(exact)))


# ---------------------------------------------------------------- against torch
@pytest.mark.parametrize("name", ["momentum", "nesterov", "dampening", "momentum0"])
def test_against_torch_on_the_gpu_within_the_float64_bar(name):
    h = dict(dict(dampening=0.0, momentum=0.0, weight_decay=0.0, nesterov=False, maximize=False), **SETTINGS[name])
    sizes = [CH + 9, 77]
    arrays, bufs, grads = draws(sizes, 11, 0.1), draws(sizes, 12, 0.3), draws(sizes, 13)
    sides = {}
    for cls in (optim.SGD, torch.optim.SGD):
        params = [torch.nn.Parameter(on_gpu(a)) for a in arrays]
        opt = cls(params, **dict(h, foreach=False))
        for p, bf, g in zip(params, bufs, grads):
            if h["momentum"]:
                opt.state[p]["momentum_buffer"] = on_gpu(bf)
            p.grad = on_gpu(g)
        opt.step()
        torch.cuda.synchronize()
        sides[cls] = [(host(p), host(opt.state[p]["momentum_buffer"]) if h["momentum"] else None) for p in params]
    for i, (a, bf, g) in enumerate(zip(arrays, bufs, grads)):
        p64, b64, M = R.sgd64(a, g, bf if h["momentum"] else None, h["lr"], h["momentum"], h["dampening"], h["weight_decay"],
                              h["nesterov"], h["maximize"])
        for cls, side in sides.items():
            rp, rb = R.bar_ratios(a, side[i][0], side[i][1], p64, b64 if h["momentum"] else None, M, h["lr"])
            assert rp <= R.BAR and rb <= R.BAR, (cls.__name__, i, rp, rb)
        want_p, want_b = R.sgd(a, g, bf if h["momentum"] else None, h["lr"], h["momentum"], h["dampening"], h["weight_decay"],
                               h["nesterov"], h["maximize"])
        assert R.same_bits(sides[optim.SGD][i][0], want_p) and (want_b is None or R.same_bits(sides[optim.SGD][i][1], want_b))


def test_state_dict_round_trip_with_torch():
    sizes = [CH + 9, 77, 3]
    h = dict(lr=0.01, momentum=0.9, weight_decay=5e-4)
    b = Beside(draws(sizes, 14, 0.1), **h)
    t_params = [torch.nn.Parameter(on_gpu(a)) for a in b.p]
    t_opt = torch.optim.SGD(t_params, foreach=False, **h)
    g0, g1, g2 = draws(sizes, 140), draws(sizes, 141), draws(sizes, 142)
    b.give(g0)
    b.opt.step()
    b.ref_step()
    # ours -> torch: torch continues from our state within the bar
    t_opt.load_state_dict(copy.deepcopy(b.opt.state_dict()))       # (load_state_dict keeps the tensors it is given: a copy each)
    with torch.no_grad():
        for tp, p in zip(t_params, b.params):
            tp.copy_(p)
    before_p, before_b = [x.copy() for x in b.p], [x.copy() for x in b.buf]
    for tp, g in zip(t_params, g1):
        tp.grad = on_gpu(g)
    t_opt.step()
    b.give(g1)
    b.opt.step()
    b.ref_step()
    b.check("after our own second step")
    for i, tp in enumerate(t_params):
        p64, b64, M = R.sgd64(before_p[i], g1[i], before_b[i], **h)
        rp, rb = R.bar_ratios(before_p[i], host(tp), host(t_opt.state[tp]["momentum_buffer"]), p64, b64, M, h["lr"])
        assert rp <= R.BAR and rb <= R.BAR, (i, rp, rb)
    # torch -> ours: we continue from torch's state, bitwise to the definition on that state
    c = Beside([host(tp) for tp in t_params], **h)
    c.opt.load_state_dict(copy.deepcopy(t_opt.state_dict()))
    c.buf = [host(t_opt.state[tp]["momentum_buffer"]).copy() for tp in t_params]
    assert all(torch.equal(c.opt.state[p]["momentum_buffer"], t_opt.state[tp]["momentum_buffer"]) for p, tp in zip(c.params, t_params))
    c.give(g2)
    c.opt.step_clipped(5.0)
    c.ref_step(5.0)
    c.check("continued from torch's state")


# ---------------------------------------------------------------- the whole net
def reference_groups(net, cls, lr, backbone_lr, wd, momentum):
    """The reference's get_optimizer with freeze_backbone False: the detection layers at lr, the backbone at backbone_lr."""
    backbone = {id(p) for p in net.feature.parameters()}
    return cls([{"params": [p for p in net.parameters() if id(p) not in backbone], "lr": lr},
                {"params": list(net.feature.parameters()), "lr": backbone_lr}], lr, weight_decay=wd, momentum=momentum)


def test_three_training_steps_of_the_80_class_net():
    hw, nc, B = (96, 96), 80, 2
    net = L.make_net(hw, nc, BF16).train()
    opt = reference_groups(net, optim.SGD, 1e-3, 1e-4, 5e-4, 0.9)
    names = {id(p): k for k, p in net.named_parameters()}
    order = [[names[id(p)] for p in g["params"]] for g in opt.param_groups]
    assert [len(o) for o in order] == [66, 156]
    named = dict(net.named_parameters())
    ref_p = {k: host(p).copy() for k, p in named.items()}
    ref_b = {k: None for k in named}
    x = L.images(B, hw, 31)
    tg = YR.random_rows(77, B, 8, nc, (0.05, 0.7))
    with torch.no_grad():                                           # the inference engine packs the initial weights
        first = net.eval().forward_cat(x.to(DEV)).clone()
    generation = net.engine().generation
    net.train()
    for k in range(3):
        GB.gpu_step(net, x, tg)
        grads = {key: host(p.grad).copy() for key, p in named.items()}
        versions = {key: p._version for key, p in named.items()}
        norm = opt.step_clipped(1000.0)
        want, coef = R.norm_and_coef([grads[key] for o in order for key in o], 1000.0)
        assert norm_bits(norm, want), (k, float(norm), float(want))
        for o, grp in zip(order, opt.param_groups):
            for key in o:
                ref_p[key], ref_b[key] = R.sgd(ref_p[key], grads[key], ref_b[key], grp["lr"], grp["momentum"], grp["dampening"],
                                               grp["weight_decay"], coef=coef)
        for key, p in named.items():
            assert R.same_bits(host(p), ref_p[key]), (k, key)
            assert R.same_bits(host(opt.state[p]["momentum_buffer"]), ref_b[key]), (k, key)
            assert p._version > versions[key], (k, key)
            assert R.same_bits(host(p.grad), grads[key]), (k, key)
    # the inference engine, packed before the first update, re-packed: the updated net's detections are those of a copy of the net that
    # was given the reference's parameters by load_state_dict
    sd = {key: v.clone() for key, v in net.state_dict().items()}
    for key in named:
        sd[key] = torch.from_numpy(ref_p[key]).view(named[key].shape)
    other = copy.deepcopy(net)
    other.load_state_dict(sd)
    net.eval()
    other.eval()
    with torch.no_grad():
        mine, theirs = net.forward_cat(x.to(DEV)), other.forward_cat(x.to(DEV))
    torch.cuda.synchronize()
    assert net.engine().generation > generation and torch.equal(mine, theirs) and not torch.equal(mine, first)


def test_a_step_on_the_heads_leaves_the_frozen_prefix_engine_packed():
    n, hw, nc = 52, (96, 96), 3
    net = FC.CUTS[n].apply(L.make_net(hw, nc, BF16))
    net.frozen_prefix = True
    trainable = [p for p in net.parameters() if p.requires_grad]
    opt = optim.SGD(trainable, lr=1e-3, momentum=0.9, weight_decay=5e-4)
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
def test_bad_tensors_raise_type_error_and_nothing_is_written():
    good = torch.nn.Parameter(on_gpu(draws([64], 15)[0]))
    start = host(good).copy()
    with pytest.raises(TypeError):
        optim.SGD([good, torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))], lr=0.1)
    cpu = torch.nn.Parameter(torch.zeros(4))
    opt = optim.SGD([good, cpu], lr=0.1, momentum=0.9)
    good.grad, cpu.grad = torch.ones_like(good), torch.ones(4)
    for call in (opt.step, lambda: opt.step_clipped(1.0), lambda: optim.clip_grad_norm_([good, cpu], 1.0)):
        with pytest.raises(TypeError):
            call()
    strided = torch.nn.Parameter(on_gpu(draws([64], 16)[0]).view(8, 8))
    opt = optim.SGD([good, strided], lr=0.1, momentum=0.9)
    strided.grad = torch.ones(8, 8, device=DEV).t()
    assert not strided.grad.is_contiguous()
    for call in (opt.step, lambda: opt.step_clipped(1.0), lambda: optim.clip_grad_norm_([good, strided], 1.0)):
        with pytest.raises(TypeError):
            call()
    torch.cuda.synchronize()
    assert R.same_bits(host(good), start) and torch.equal(good.grad, torch.ones_like(good)) and not opt.state.get(good)
    with pytest.raises(ValueError):
        optim.clip_grad_norm_([good], 1.0, norm_type=1)
    assert float(optim.clip_grad_norm_([], 1.0)) == 0.0
