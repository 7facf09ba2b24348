"""The update step without a GPU: the numpy definition (tests/optim_ref.py) against float64 and against torch's CPU SGD, the norm's
accuracy, and the optimizer contract of yolo_v3_amd.optim.SGD (defaults, param groups, state_dict interchange, argument checks)."""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from yolo_v3_amd import YoloNet, _ffi, optim

N = 1000003               # 62 chunks, the last one short and odd
HYPER = dict(lr=1e-3, momentum=0.9, dampening=0.0, weight_decay=5e-4)


def state(seed=0, n=N):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(np.float32) * s for s in (0.05, 0.3, 1.0)]     # p, buf, g


def test_chunk_constants_agree():
    assert optim.CHUNK == R.CHUNK == _ffi.lib().yv3_optim_chunk()
    assert R.CHUNK % (R.THREADS * 4) == 0


def test_reference_step_is_within_the_float64_bar_with_the_clip_active():
    p, buf, g = state()
    total_norm, coef = R.norm_and_coef([g], 10.0)
    assert 0 < coef < 1 and abs(float(total_norm) - 1000.0) < 5
    coef64 = min(10.0 / (math.sqrt(math.fsum(np.square(g.astype(np.float64)))) + 1e-6), 1.0)
    p1, buf1 = R.sgd(p, g, buf, coef=coef, **HYPER)
    p64, buf64, M = R.sgd64(p, g, buf, coef=coef64, **HYPER)
    rp, rb = R.bar_ratios(p, p1, buf1, p64, buf64, M, HYPER["lr"])
    print("clipped step vs float64: p %.2f, buf %.2f half-ulps of the bar's scale (bar %.0f)" % (rp, rb, R.BAR))
    assert rp <= R.BAR and rb <= R.BAR


@pytest.mark.parametrize("extra", [dict(), dict(nesterov=True), dict(dampening=0.1), dict(maximize=True), dict(weight_decay=0.0),
                                   dict(momentum=0.0)], ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()) or "plain")
def test_torch_cpu_sgd_and_the_reference_are_within_the_float64_bar(extra):
    """Two steps (the first creates the buffer) of torch.optim.SGD(foreach=False) on the CPU, no clip: torch's definition and this one agree."""
    h = dict(HYPER, **extra)
    p, _, g = state(1, 70001)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.SGD([tp], foreach=False, **h)
    rp_ref, buf_ref, p64, buf64 = p, None, p.astype(np.float64), None
    for k in range(2):
        gk = (g * np.float32(1 + k)).astype(np.float32)
        tp.grad = torch.from_numpy(gk.copy())
        before = tp.detach().numpy().copy()
        opt.step()
        t64, tb64, M = R.sgd64(before, gk, buf64 if k else None, **h)
        tbuf = opt.state[tp]["momentum_buffer"].numpy() if h["momentum"] else None
        rp, rb = R.bar_ratios(before, tp.detach().numpy(), tbuf, t64, tb64, M, h["lr"])
        assert rp <= R.BAR and rb <= R.BAR, ("torch", k, rp, rb)
        buf64 = tbuf.astype(np.float64) if tbuf is not None else None
        r64, rb64, M = R.sgd64(rp_ref, gk, buf_ref, **h)
        new_p, new_buf = R.sgd(rp_ref, gk, buf_ref, **h)
        rp, rb = R.bar_ratios(rp_ref, new_p, new_buf, r64, rb64, M, h["lr"])
        assert rp <= R.BAR and rb <= R.BAR, ("reference", k, rp, rb)
        rp_ref, buf_ref = new_p, new_buf
    if not h["momentum"]:
        assert buf_ref is None and "momentum_buffer" not in opt.state[tp]


def test_total_norm_is_the_float64_norm_to_one_fp32_ulp():
    g = state(2)[2]
    exact = math.sqrt(math.fsum(np.square(g.astype(np.float64))))
    total_norm, _ = R.norm_and_coef([g[:300000], g[300000:300001], g[300001:]], 1e9)       # three tensors, one of one element
    assert total_norm.dtype == np.float32
    assert abs(float(total_norm) - exact) <= float(np.spacing(np.float32(exact)))
    assert float(R.sum_of_squares([])) == 0.0 and R.norm_and_coef([], 5.0) == (0.0, 1.0)
    t = torch.nn.Parameter(torch.zeros(g.size))
    t.grad = torch.from_numpy(g.copy())
    theirs = float(torch.nn.utils.clip_grad_norm_([t], 1e9))
    print("relative deviation from the float64 norm at %d elements: ours %.2g, torch (CPU) %.2g"
          % (g.size, (float(total_norm) - exact) / exact, (theirs - exact) / exact))


def test_non_finite_gradients_follow_torch():
    g = np.array([1.0, np.inf, -2.0], dtype=np.float32)
    total_norm, coef = R.norm_and_coef([g], 1.0)
    assert np.isinf(total_norm) and coef == 0.0
    assert np.isnan(R.scale(g, coef)[1]) and R.scale(g, coef)[0] == 0.0
    g[1] = np.nan
    total_norm, coef = R.norm_and_coef([g], 1.0)
    assert np.isnan(total_norm) and np.isnan(coef)                 # (torch.clamp keeps the NaN)
    assert R.same_bits(R.scale(g, coef), np.full(3, np.nan, dtype=np.float32))


def test_defaults_and_signature_are_torchs():
    ours = optim.SGD([torch.nn.Parameter(torch.zeros(3))])
    theirs = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))])
    assert list(ours.defaults) == list(theirs.defaults)
    assert {k: v for k, v in ours.defaults.items() if k not in ("foreach", "differentiable", "fused")} == \
           {k: v for k, v in theirs.defaults.items() if k not in ("foreach", "differentiable", "fused")}
    so, st = inspect.signature(optim.SGD.__init__), inspect.signature(torch.optim.SGD.__init__)
    assert [(p.name, p.kind, p.default) for p in so.parameters.values()] == [(p.name, p.kind, p.default) for p in st.parameters.values()]
    for bad in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError):
            optim.SGD([torch.nn.Parameter(torch.zeros(3))], **bad)
        with pytest.raises(ValueError):
            torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], **bad)


def two_groups(net, cls, lr, backbone_lr, wd, momentum, freeze_backbone):
    """The reference's get_optimizer (train.py): the detection layers at lr, the backbone at backbone_lr or frozen."""
    backbone = {id(p) for p in net.feature.parameters()}
    groups = [{"params": [p for p in net.parameters() if id(p) not in backbone], "lr": lr}]
    if freeze_backbone:
        for p in net.feature.parameters():
            p.requires_grad = False
    else:
        groups.append({"params": list(net.feature.parameters()), "lr": backbone_lr})
    return cls(groups, lr, weight_decay=wd, momentum=momentum)


@pytest.mark.parametrize("freeze", [False, True])
def test_the_references_two_groups_build_and_exchange_state_dicts(freeze):
    net = YoloNet((96, 96), numClass=80)
    ours, theirs = (two_groups(net, cls, 1e-3, 1e-4, 5e-4, 0.9, freeze) for cls in (optim.SGD, torch.optim.SGD))
    assert len(ours.param_groups) == (1 if freeze else 2)
    assert [[id(p) for p in g["params"]] for g in ours.param_groups] == [[id(p) for p in g["params"]] for g in theirs.param_groups]
    assert sum(len(g["params"]) for g in ours.param_groups) == (222 - 156 if freeze else 222)
    for go, gt in zip(ours.param_groups, theirs.param_groups):
        assert {k: v for k, v in go.items() if k != "params"} == {k: v for k, v in gt.items() if k != "params"}
    heads = ours.param_groups[0]["params"][:3]
    for p in heads:                                                # torch steps three tensors on the CPU: a state to hand over
        p.grad = torch.ones_like(p)
    theirs.step()
    sd = theirs.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2]
    ours.load_state_dict(sd)
    for p in heads:
        assert torch.equal(ours.state[p]["momentum_buffer"], theirs.state[p]["momentum_buffer"])
    back = torch.optim.SGD([{"params": g["params"]} for g in ours.param_groups], 0.5)
    back.load_state_dict(ours.state_dict())
    assert back.param_groups[0]["lr"] == 1e-3 and back.param_groups[0]["momentum"] == 0.9
    assert all(torch.equal(back.state[p]["momentum_buffer"], ours.state[p]["momentum_buffer"]) for p in heads)
    sched = torch.optim.lr_scheduler.StepLR(ours, step_size=1, gamma=0.5)
    assert sched.get_last_lr()[0] == 1e-3


def test_bad_tensors_raise_type_error_before_anything_is_launched():
    with pytest.raises(TypeError):
        optim.SGD([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))], lr=0.1)
    with pytest.raises(TypeError):
        optim.SGD([torch.nn.Parameter(torch.zeros(4, 4).t())], lr=0.1)
    p = torch.nn.Parameter(torch.zeros(4))                        # a CPU parameter: refused when it would be updated
    opt = optim.SGD([p], lr=0.1)
    opt.step()                                                     # (no .grad: nothing to do, as in torch)
    p.grad = torch.ones(4)
    for call in (opt.step, lambda: opt.step_clipped(1.0), lambda: optim.clip_grad_norm_([p], 1.0)):
        with pytest.raises(TypeError):
            call()
    assert torch.equal(p.detach(), torch.zeros(4)) and torch.equal(p.grad, torch.ones(4)) and not opt.state[p]
    with pytest.raises(ValueError):
        optim.clip_grad_norm_([p], 1.0, norm_type=1.0)
    with pytest.raises(ValueError):
        optim.clip_grad_norm_([p], 1.0, norm_type=float("inf"))
    p.grad = None
    assert float(optim.clip_grad_norm_([p], 1.0)) == 0.0 and float(optim.clip_grad_norm_([], 1.0)) == 0.0


def test_entry_points_check_their_arguments_before_they_launch():
    lib, E = _ffi.lib(), _ffi.EINVAL
    import ctypes
    ptr, n = (ctypes.c_void_p * 1)(64), (ctypes.c_longlong * 1)(8)
    null, zero = (ctypes.c_void_p * 1)(None), (ctypes.c_longlong * 1)(0)
    assert lib.yv3_grad_sumsq(ptr, n, -1, 64, 1, None) == E and lib.yv3_grad_sumsq(null, n, 1, 64, 1, None) == E
    assert lib.yv3_grad_sumsq(ptr, zero, 1, 64, 1, None) == E and lib.yv3_grad_sumsq(ptr, n, 1, None, 1, None) == E
    assert lib.yv3_grad_sumsq(ptr, n, 1, 64, 0, None) == _ffi.EWORKSPACE
    assert lib.yv3_clip_coef(None, 1, 1.0, 64, None) == E and lib.yv3_clip_coef(64, 1, 1.0, None, None) == E
    assert lib.yv3_grad_scale(ptr, n, 1, None, None) == E and lib.yv3_grad_scale(null, n, 1, 64, None) == E
    assert lib.yv3_sgd_step(null, ptr, ptr, n, 1, None, 0.1, 0.9, 1.0, 0.0, 0, None) == E
    assert lib.yv3_sgd_step(ptr, null, ptr, n, 1, None, 0.1, 0.9, 1.0, 0.0, 0, None) == E
    assert lib.yv3_sgd_step(ptr, ptr, None, n, 1, None, 0.1, 0.9, 1.0, 0.0, 0, None) == E          # momentum without buffers
    assert lib.yv3_sgd_step(ptr, ptr, ptr, n, 1, None, 0.1, 0.9, 1.0, 0.0, 8, None) == E           # an unknown flag
    assert lib.yv3_sgd_step(ptr, ptr, ptr, zero, 1, None, 0.1, 0.9, 1.0, 0.0, 0, None) == E
    assert lib.yv3_sgd_step(None, None, None, None, 0, None, 0.1, 0.9, 1.0, 0.0, 0, None) == 0      # an empty list: nothing to launch
