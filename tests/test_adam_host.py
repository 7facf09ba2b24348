"""Adam / AdamW without a GPU: the numpy definition (tests/adam_ref.py) against float64 and against torch's CPU Adam / AdamW within
the bar, and the optimizer contract of yolo_v3_amd.optim.Adam / AdamW (signature, defaults, param groups, state_dict keys, a
scheduler, the refusals, argument checks of yv3_adam_step)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import optim_ref as R
from tests.test_optim_host import two_groups
from yolo_v3_amd import YoloNet, _ffi, optim
import yolo_v3_amd

N = 100003
STEPS = 4


def start(seed=0, n=N):
    return (np.random.default_rng(seed).standard_normal(n) * 0.05).astype(np.float32)


def torch_kwargs(h):
    """tests/adam_ref.py's keyword names -> torch's."""
    h = dict(h)
    h.pop("decoupled", None)
    return h


@pytest.mark.parametrize("coef", [None, 0.37], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("name", sorted(A.SETTINGS))
def test_the_definition_is_within_the_float64_bar(name, coef):
    """Four steps; each step's fp32 result against the float64 step from the same fp32 state, every element in the maximum."""
    h = A.SETTINGS[name]
    p, m, v, x = start(1), None, None, None
    worst = [0.0, 0.0, 0.0]
    for k in range(STEPS):
        g = A.wide_draws(N, 10 + k)
        c = coef if k % 2 == 0 else None                            # every other step clipped
        new = A.adam(p, g, m, v, x, k + 1, coef=c, **h)
        p64, m64, v64, _, scales = A.adam64(p, g, m, v, x, k + 1, coef=1.0 if c is None else float(np.float32(c)), **h)
        ratios = A.bar_ratios(new[:3], (p64, m64, v64), scales)
        worst = [max(a, b) for a, b in zip(worst, ratios)]
        p, m, v, x = new
        assert (x is not None) == bool(h.get("amsgrad"))
    print("%s: max ratios p %.2f, m %.2f, v %.2f of the bar's scale (K = %.0f)" % ((name,) + tuple(worst) + (A.K,)))
    assert max(worst) <= A.K, worst
    gg, bgg = g * g, (np.float32(0.001) * g) * g
    assert np.count_nonzero(g) < g.size and np.any((gg > 0) & (gg < 1.2e-38)) and np.any((bgg == 0) & (g != 0))   # subnormal, and flushed by rounding


def test_lerp_takes_both_branches_and_the_first_step_reads_no_state():
    p, g = start(2, 1001), A.wide_draws(1001, 3)
    for betas, low in (((0.9, 0.999), True), ((0.4, 0.99), False), ((0.0, 0.999), False)):
        w = np.float32(1 - betas[0])
        assert (abs(w) < 0.5) == low
        first = A.adam(p, g, None, None, None, 1, betas=betas, amsgrad=True)
        zeros = np.zeros_like(p)
        again = A.adam(p, g, zeros, zeros, zeros, 1, betas=betas, amsgrad=True)
        assert all(R.same_bits(a, b) for a, b in zip(first, again))
    # L2 decay is decided on the fp32 scalar: a weight_decay that rounds to 0 in fp32 is no decay (p = inf adds no 0 * inf = NaN to g)
    gz, pz = np.array([-0.0, 1.0], dtype=np.float32), np.array([1.0, np.inf], dtype=np.float32)
    assert all(R.same_bits(a, b) for a, b in zip(A.adam(pz, gz, None, None, None, 1, weight_decay=1e-46)[:3], A.adam(pz, gz, None, None, None, 1)[:3]))
    assert np.isinf(A.adam(pz, gz, None, None, None, 1, weight_decay=1e-46)[0][1]) and np.isnan(A.adam(pz, gz, None, None, None, 1, weight_decay=1e-44)[0][1])
    nan = A.maximum(np.array([np.nan, 1.0, 2.0], dtype=np.float32), np.array([1.0, np.nan, 1.0], dtype=np.float32))
    assert np.isnan(nan[0]) and np.isnan(nan[1]) and nan[2] == 2.0


@pytest.mark.parametrize("name", sorted(A.SETTINGS))
def test_torch_cpu_adam_is_within_the_same_bar(name):
    """torch.optim.Adam / AdamW(foreach=False) on the CPU, four steps: torch's kernels fuse and reorder, so the bar, not the bits."""
    h = A.SETTINGS[name]
    cls = torch.optim.AdamW if h.get("decoupled") else torch.optim.Adam
    tp = torch.nn.Parameter(torch.from_numpy(start(4, 20011).copy()))
    opt = cls([tp], foreach=False, **torch_kwargs(h))
    worst = [0.0, 0.0, 0.0]
    for k in range(STEPS):
        g = A.wide_draws(tp.numel(), 40 + k)
        st = opt.state[tp]
        before = [tp.detach().numpy().copy()] + [st[key].numpy().copy() if key in st else None
                                                 for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")]
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        assert float(st["step"]) == k + 1
        p64, m64, v64, _, scales = A.adam64(before[0], g, before[1], before[2], before[3], k + 1, **h)
        got = (tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy())
        worst = [max(a, b) for a, b in zip(worst, A.bar_ratios(got, (p64, m64, v64), scales))]
    print("torch CPU %s: max ratios p %.2f, m %.2f, v %.2f (K = %.0f)" % ((name,) + tuple(worst) + (A.K,)))
    assert max(worst) <= A.K, worst


# ---------------------------------------------------------------- the optimizer contract
def one():
    return [torch.nn.Parameter(torch.zeros(3))]


@pytest.mark.parametrize("ours,theirs", [(optim.Adam, torch.optim.Adam), (optim.AdamW, torch.optim.AdamW)])
def test_defaults_and_signature_are_torchs(ours, theirs):
    assert yolo_v3_amd.Adam is optim.Adam and yolo_v3_amd.AdamW is optim.AdamW and issubclass(optim.AdamW, optim.Adam)
    a, b = ours(one()), theirs(one())
    assert list(a.defaults) == list(b.defaults) and a.defaults == b.defaults
    assert a.defaults["decoupled_weight_decay"] == (ours is optim.AdamW)
    sa, sb = inspect.signature(ours.__init__), inspect.signature(theirs.__init__)
    assert [(p.name, p.kind, p.default) for p in sa.parameters.values()] == [(p.name, p.kind, p.default) for p in sb.parameters.values()]
    for key in a.param_groups[0]:
        if key != "params":
            assert a.param_groups[0][key] == b.param_groups[0][key], key
    assert list(a.param_groups[0]) == list(b.param_groups[0])
    for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1e-4)):
        for cls in (ours, theirs):
            with pytest.raises(ValueError):
                cls(one(), **bad)
    for harmless in (dict(foreach=True), dict(fused=True), dict(differentiable=True), dict(lr=torch.tensor(0.01))):
        ours(one(), **harmless)


def test_what_would_need_a_device_read_is_refused():
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(ValueError):
            cls(one(), capturable=True)
        with pytest.raises(ValueError):
            cls(one(), betas=(torch.tensor(0.9), torch.tensor(0.999)))
        with pytest.raises(ValueError):
            cls(one(), lr=torch.tensor([0.1, 0.2]))
        with pytest.raises(ValueError):
            cls(one(), lr=torch.empty(1, device="meta"))              # stands in for a GPU tensor: any device but the CPU
        opt = cls(one())
        opt.param_groups[0]["capturable"] = True                      # set after construction: refused by the step
        opt.param_groups[0]["params"][0].grad = torch.ones(3)
        with pytest.raises(ValueError):
            opt.step()
        opt.param_groups[0]["capturable"] = False
        opt.param_groups[0]["betas"] = (torch.tensor(0.9), 0.999)
        with pytest.raises(ValueError):
            opt.step()
        assert not opt.state


def test_bad_tensors_raise_type_error_before_anything_is_launched():
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(TypeError):
            cls([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
        with pytest.raises(TypeError):
            cls([torch.nn.Parameter(torch.zeros(4, 4).t())])
        p = torch.nn.Parameter(torch.zeros(4))                        # a CPU parameter: refused when it would be updated
        opt = cls([p])
        opt.step()                                                    # (no .grad: nothing to do, as in torch)
        assert opt.step_clipped(1.0) == 0.0 and not opt.state
        p.grad = torch.ones(4)
        for call in (opt.step, lambda: opt.step_clipped(1.0)):
            with pytest.raises(TypeError):
                call()
        assert torch.equal(p.detach(), torch.zeros(4)) and not opt.state.get(p)


def test_the_references_two_groups_and_the_state_dict_keys():
    net = YoloNet((96, 96), numClass=80)
    pair = []
    for cls in (optim.AdamW, torch.optim.AdamW):
        backbone = {id(p) for p in net.feature.parameters()}
        pair.append(cls([{"params": [p for p in net.parameters() if id(p) not in backbone], "lr": 1e-3},
                         {"params": list(net.feature.parameters()), "lr": 1e-4}], 1e-3, weight_decay=5e-4, amsgrad=True))
    ours, theirs = pair
    assert [len(g["params"]) for g in ours.param_groups] == [66, 156]
    for go, gt in zip(ours.param_groups, theirs.param_groups):
        assert {k: v for k, v in go.items() if k != "params"} == {k: v for k, v in gt.items() if k != "params"}
    heads = ours.param_groups[0]["params"][:3]
    for p in heads:                                                   # torch steps three tensors on the CPU: a state to hand over
        p.grad = torch.ones_like(p)
    theirs.step()
    sd = theirs.state_dict()
    ours.load_state_dict(sd)
    mine = ours.state_dict()
    assert mine["state"].keys() == sd["state"].keys() and list(mine["state"][0]) == ["step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"]
    assert [sorted(g) for g in mine["param_groups"]] == [sorted(g) for g in sd["param_groups"]]
    for p in heads:
        st = ours.state[p]
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 1
        assert torch.equal(st["exp_avg"], theirs.state[p]["exp_avg"])
    back = torch.optim.AdamW([{"params": g["params"]} for g in ours.param_groups])
    back.load_state_dict(mine)
    assert back.param_groups[1]["lr"] == 1e-4 and back.param_groups[0]["amsgrad"] is True
    # SGD's helper builds the same two groups for any class that takes (groups, lr, weight_decay=, momentum=): Adam does not take momentum
    assert len(two_groups(net, optim.SGD, 1e-3, 1e-4, 5e-4, 0.9, False).param_groups) == 2


def test_a_scheduler_moves_the_learning_rate_the_step_reads():
    opt = optim.Adam(one(), lr=0.1)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    opt.step()
    sched.step()
    assert opt.param_groups[0]["lr"] == 0.05 and sched.get_last_lr() == [0.05]
    assert optim._adam_hyper(opt.param_groups[0])[0] == 0.05
    state = opt.__getstate__()
    state["state"] = {opt.param_groups[0]["params"][0]: dict(step=3, exp_avg=torch.zeros(3), exp_avg_sq=torch.zeros(3))}
    opt.__setstate__(state)                                           # an old checkpoint's integer step becomes torch's CPU tensor
    step = opt.state[opt.param_groups[0]["params"][0]]["step"]
    assert torch.is_tensor(step) and step.dtype == torch.float32 and float(step) == 3


def test_the_entry_point_checks_its_arguments_before_it_launches():
    lib, E = _ffi.lib(), _ffi.EINVAL
    ptr, n = (ctypes.c_void_p * 1)(64), (ctypes.c_longlong * 1)(8)
    null, zero = (ctypes.c_void_p * 1)(None), (ctypes.c_longlong * 1)(0)
    sc = (0.1, 0.999, 0.001, 0.03, 1e-8, -0.001, 0.0)

    def call(p=ptr, g=ptr, m=ptr, v=ptr, x=ptr, sizes=n, count=1, flags=0):
        return lib.yv3_adam_step(p, g, m, v, x, sizes, count, None, *sc, flags, None)

    for which in ("p", "g", "m", "v"):
        assert call(**{which: null}) == E and call(**{which: None}) == E
    assert call(x=None, flags=2) == E and call(x=null, flags=2) == E             # amsgrad without its state
    assert call(flags=16) == E and call(flags=-1) == E                            # unknown flags
    assert call(sizes=zero) == E and call(sizes=None) == E and call(count=-1) == E
    assert call(sizes=(ctypes.c_longlong * 1)(-5)) == E
    assert call(sizes=(ctypes.c_longlong * 1)((2 ** 30 + 1) * optim.CHUNK)) == _ffi.ELIMIT
    assert lib.yv3_adam_step(None, None, None, None, None, None, 0, None, *sc, 0, None) == 0      # an empty list: nothing to launch
    assert (optim._ADAM_FIRST, optim._ADAM_AMSGRAD, optim._ADAM_MAXIMIZE, optim._ADAM_DECOUPLED) == (1, 2, 4, 8)
