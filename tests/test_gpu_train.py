"""Backprop of the YOLO loss into every parameter (net.backprop = True; yolo_v3_amd/backprop.py, csrc/train.hip) against the float64
restatement tests/train_ref.py, plus the C-ABI of the training kernels against float64, one layer shape at a time.

Precision bars.  Whole-step checks compare each gradient's and running statistic's relative L2 error against float64 with one bar per
case: BAR_FACTOR times the largest such error of the same step run by torch in fp32 on the CPU (train_ref with dtype=float32).  A
train-mode step is ill-conditioned where a channel's batch variance is small or a pre-activation sits near 0 (LeakyReLU's kink), and
there the error of any fp32 implementation depends on its summation order (the GPU's fp32 MFMA chains sum in k order, the CPU's
blocked kernels pairwise), so the bar is set by the worst tensor rather than per tensor; a wrong gradient is off by O(1).  Kernel checks bound each element by the fp32 error model of an fp32 MFMA
chain / fp32 elementwise op (see the constants below)."""
import copy
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_train_host as H
from tests import train_ref as T
from tests import yolo_loss_ref as R
from tests.helpers import trained_like_stream
from yolo_v3_amd import YoloNet, WeightManager, _ffi, arch, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR_FACTOR = 16.0      # every tensor's GPU rel-L2 error <= BAR_FACTOR * the largest per-tensor rel-L2 error of torch fp32 on the CPU


def make_net(size, C, stream=None):
    net = YoloNet((size, size), numClass=C)
    WeightManager(net).load_stream(stream if stream is not None else trained_like_stream(C))
    return net.to(DEV)


def pick_target(logits, size, C, B, T_rows, seed):
    """Target rows whose decisions all clear the 1e-4 margins on the float64 logits."""
    for attempt in range(100):
        tg = R.random_rows(seed * 1000 + attempt, B, T_rows, C, (0.03, 0.8), n_valid_lo=3)
        res = T.head_losses(logits, tg, size, C)
        if all(R.margins_ok(r["margins"]) for r in res) and sum(r["nGT"] for r in res) > 0:
            return tg
    raise AssertionError("no target draw clears the margins")


def gpu_step(net, x, tg):
    net.backprop = True
    for p in net.parameters():
        p.grad = None
    loss = net(x.to(DEV), torch.as_tensor(tg))
    loss.backward()
    torch.cuda.synchronize()
    return loss


def check_against_ref(net_before_sd, net, loss, x, tg, C, train):
    ref = T.run(net_before_sd, x, tg, C, train=train)
    ref32 = T.run(net_before_sd, x, tg, C, train=train, dtype=torch.float32)
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert net.stats["nGT"] == ref["stats"][8] and net.stats["nCorrect"] == ref["stats"][7]
    worst = []
    named = dict(net.named_parameters())
    for k, g64 in ref["grads"].items():
        g = named[k].grad
        assert g is not None and torch.isfinite(g).all(), k
        e, e32 = T.rel_l2(g.cpu(), g64), T.rel_l2(ref32["grads"][k], g64)
        worst.append((None, k, e, e32))
    mods = dict(net.named_modules())
    for prefix, (m64, v64) in ref["running"].items():
        bn = mods[prefix].bn
        for name, got, r64, r32 in (("mean", bn.running_mean, m64, ref32["running"][prefix][0]),
                                    ("var", bn.running_var, v64, ref32["running"][prefix][1])):
            e, e32 = T.rel_l2(got.cpu(), r64), T.rel_l2(r32, r64)
            worst.append((None, prefix + ".running_" + name, e, e32))
    bar = BAR_FACTOR * max(e32 for _, _, _, e32 in worst)
    worst.sort(key=lambda t: -t[2])
    print("bar %.3g; largest GPU errors (tensor, GPU, fp32 CPU):" % bar, [(k, "%.3g" % e, "%.3g" % e32) for _, k, e, e32 in worst[:4]])
    assert worst[0][2] <= bar, (bar, worst[:4])
    return ref


# ---------------------------------------------------------------- whole step against float64
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_fixture_step_matches_float64(train):
    """The case of tests/golden/train_step.npz (the reference's own step; tests/test_train_host.py pins train_ref to it)."""
    sd, x, tg, _ = H.case()
    C, size = H.CASE["C"], H.CASE["size"]
    net = make_net(size, C)
    net.train(train)
    x = torch.from_numpy(x)
    loss = gpu_step(net, x, tg)
    assert loss.requires_grad
    gold = np.load(H.GOLD)
    mode = "train" if train else "eval"
    assert abs(float(loss.detach()) - float(gold[mode + "/loss"])) <= 1e-5 * abs(float(gold[mode + "/loss"]))
    check_against_ref(sd, net, loss, x, tg, C, train)
    nbt = int(net.feature.mlist[0].bn.num_batches_tracked)
    assert nbt == (1 if train else 0)


def test_416_step_matches_float64():
    C, size, B = 80, 416, 4
    net = make_net(size, C).train()
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = torch.from_numpy(synth.images(B, size, 511))
    logits, _, _ = T.forward(sd, x, True)
    tg = pick_target(logits, size, C, B, 20, 43)
    loss = gpu_step(net, x, tg)
    check_against_ref(sd, net, loss, x, tg, C, True)


# ---------------------------------------------------------------- semantics
def _fixture_case(train=True):
    C, size, B = 3, 96, 2
    net = make_net(size, C).train(train)
    x = torch.from_numpy(synth.images(B, size, 31))
    tg = R.random_rows(77, B, 8, C, (0.05, 0.7))
    return net, x, tg


def _grads(net):
    return {k: (p.grad.clone() if p.grad is not None else None) for k, p in net.named_parameters()}


def test_steps_are_bitwise_deterministic():
    net, x, tg = _fixture_case()
    a, b = copy.deepcopy(net), copy.deepcopy(net)
    la, lb = gpu_step(a, x, tg), gpu_step(b, x, tg)
    assert float(la) == float(lb)
    ga, gb = _grads(a), _grads(b)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for (k, t1), (_, t2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(t1, t2), k


def test_backward_accumulates():
    net, x, tg = _fixture_case(train=False)
    gpu_step(net, x, tg)
    g1 = _grads(net)
    net(x.to(DEV), torch.as_tensor(tg)).backward(torch.tensor(0.5, device=DEV))
    torch.cuda.synchronize()
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, g1[k] + g1[k] * 0.5), k


def test_frozen_backbone_stops_at_the_heads():
    net, x, tg = _fixture_case()
    full, frozen = copy.deepcopy(net), copy.deepcopy(net)
    for n, p in frozen.named_parameters():
        if n.startswith("feature."):
            p.requires_grad_(False)
    gpu_step(full, x, tg)
    gpu_step(frozen, x, tg)
    gf = dict(full.named_parameters())
    for n, p in frozen.named_parameters():
        if n.startswith("feature."):
            assert p.grad is None, n
        else:
            assert torch.equal(p.grad, gf[n].grad), n


def test_sgd_reduces_the_loss_and_the_engine_sees_the_weights():
    net, x, tg = _fixture_case()
    with torch.no_grad():                  # an inference engine with packed weights exists before the optimizer moves them
        before = net.eval().forward_cat(x.to(DEV)).clone()
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9)
    net.backprop = True
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = net(x.to(DEV), torch.as_tensor(tg))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1000)
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses
    net.eval()
    fresh = YoloNet((96, 96), numClass=3).to(DEV)
    fresh.load_state_dict(net.state_dict())
    fresh.eval()
    with torch.no_grad():
        a, b = net.forward_cat(x.to(DEV)), fresh.forward_cat(x.to(DEV))
    assert torch.equal(a, b) and not torch.equal(a, before)


def test_backprop_off_keeps_the_no_grad_loss():
    net, x, tg = _fixture_case(train=False)
    ref = copy.deepcopy(net)
    loss = net(x.to(DEV), torch.as_tensor(tg))
    assert not loss.requires_grad and net.backprop is False
    assert float(loss) == float(ref._loss(x.to(DEV), torch.as_tensor(tg)))
    assert all(p.grad is None for p in net.parameters())


def test_input_gradient_raises():
    net, x, tg = _fixture_case()
    net.backprop = True
    with pytest.raises(NotImplementedError):
        net(x.to(DEV).requires_grad_(True), torch.as_tensor(tg))


# ---------------------------------------------------------------- C-ABI, one distinct layer shape at a time
CONV_BAR = 2e-6        # |got - ref| <= CONV_BAR * sum|a b| (fp32 MFMA chain: ~1e-7 * sum|a b| per 1k terms, guide measurements)
CANARY = 64


def _buf(n):
    return torch.full((n + CANARY,), float("nan"), device=DEV, dtype=torch.float32)


def _canary_ok(b, n):
    return bool(torch.isnan(b[n:]).all())


def _shapes(size=64):
    out, seen = [], set()
    for sp, (ho, wo) in zip(arch.conv_specs(80), arch.conv_output_hw(size, 80)):
        cin_up = {"pre_det2.mlist.0": 256, "pre_det3.mlist.0": 128}.get(sp.name, 0)
        key = (sp.cin, sp.cout, sp.k, sp.stride, cin_up, ho)
        if key not in seen:
            seen.add(key)
            out.append(dict(name=sp.name, cin=sp.cin, cout=sp.cout, k=sp.k, stride=sp.stride, cin_up=cin_up, H=ho * sp.stride))
    return out


SHAPES = _shapes()


def _close(got, ref, scale, bar, what):
    d = (got.double().cpu() - ref).abs()
    assert torch.isfinite(got).all(), what + ": non-finite"
    worst = float((d / (scale + 1e-30)).max())
    assert worst <= bar, "%s: %.3g > %.3g" % (what, worst, bar)


@pytest.mark.parametrize("sh", SHAPES, ids=[s["name"] for s in SHAPES])
def test_conv_kernels_per_shape(sh):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    B, H, cin, cout, k, st, cu = 2, sh["H"], sh["cin"], sh["cout"], sh["k"], sh["stride"], sh["cin_up"]
    W, nchw = H, int(cin == 3)
    g = torch.Generator().manual_seed(zlib.crc32(sh["name"].encode()))
    x64 = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64).float().double()
    w64 = (torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / np.sqrt(cin * k * k)).float().double()
    pad = (k - 1) // 2
    # the cin_up form's input: channels [0, cu) are up2x of a low-resolution map
    if cu:
        low = torch.randn(B, cu, H // 2, W // 2, generator=g, dtype=torch.float64).float().double()
        x64[:, :cu] = F.interpolate(low, scale_factor=2, mode="nearest")
        xin = x64[:, cu:].permute(0, 2, 3, 1).contiguous().float().to(DEV)
        x2 = low.permute(0, 2, 3, 1).contiguous().float().to(DEV)
    else:
        xin = (x64 if nchw else x64.permute(0, 2, 3, 1)).contiguous().float().to(DEV)
        x2 = None
    x2p = x2.data_ptr() if x2 is not None else None
    wd = w64.float().contiguous().to(DEV)
    wf, wdd = _buf(wd.numel()), _buf(wd.numel())
    _ffi.check(lib.yv3_train_pack_weight(wd.data_ptr(), wf.data_ptr(), wdd.data_ptr(), cout, cin, k, s))
    # forward
    z64 = F.conv2d(x64, w64, stride=st, padding=pad)
    za = F.conv2d(x64.abs(), w64.abs(), stride=st, padding=pad)
    Ho = z64.shape[2]
    nz = B * Ho * Ho * cout
    z = _buf(nz)
    _ffi.check(lib.yv3_train_conv_fwd(xin.data_ptr(), x2p, wf.data_ptr(), None, z.data_ptr(), B, H, W, cin, cu, cout, k, st, nchw, s))
    torch.cuda.synchronize()
    assert _canary_ok(z, nz)
    _close(z[:nz].view(B, Ho, Ho, cout), z64.permute(0, 2, 3, 1), za.permute(0, 2, 3, 1), CONV_BAR, "fwd")
    # dgrad (on the full cin; the cin_up split is yv3_train_upcat_bwd) and wgrad
    dz64 = torch.randn(B, cout, Ho, Ho, generator=g, dtype=torch.float64).float().double()
    dzd = dz64.permute(0, 2, 3, 1).contiguous().float().to(DEV)
    if not nchw:
        nx = B * H * W * cin
        dx = _buf(nx)
        _ffi.check(lib.yv3_train_conv_dgrad(dzd.data_ptr(), wdd.data_ptr(), dx.data_ptr(), B, H, W, cin, cout, k, st, 0, s))
        torch.cuda.synchronize()
        assert _canary_ok(dx, nx)
        ref = torch.nn.grad.conv2d_input(x64.shape, w64, dz64, stride=st, padding=pad)
        sc = torch.nn.grad.conv2d_input(x64.shape, w64.abs(), dz64.abs(), stride=st, padding=pad)
        _close(dx[:nx].view(B, H, W, cin), ref.permute(0, 2, 3, 1), sc.permute(0, 2, 3, 1), CONV_BAR, "dgrad")
    nb = lib.yv3_train_conv_wgrad_workspace_bytes(B, H, W, cin, cout, k, st)
    assert nb > 0
    ws = torch.empty(nb, device=DEV, dtype=torch.uint8)
    nw = wd.numel()
    dw = _buf(nw)
    assert lib.yv3_train_conv_wgrad(xin.data_ptr(), x2p, dzd.data_ptr(), dw.data_ptr(), B, H, W, cin, cu, cout, k, st, nchw,
                                    ws.data_ptr(), nb - 1, s) == _ffi.EWORKSPACE
    _ffi.check(lib.yv3_train_conv_wgrad(xin.data_ptr(), x2p, dzd.data_ptr(), dw.data_ptr(), B, H, W, cin, cu, cout, k, st, nchw,
                                        ws.data_ptr(), nb, s))
    torch.cuda.synchronize()
    assert _canary_ok(dw, nw)
    ref = torch.nn.grad.conv2d_weight(x64, w64.shape, dz64, stride=st, padding=pad)
    sc = torch.nn.grad.conv2d_weight(x64.abs(), w64.shape, dz64.abs(), stride=st, padding=pad)
    _close(dw[:nw].view_as(w64), ref, sc, CONV_BAR, "wgrad")


BN_C = sorted({sp.cout for sp in arch.conv_specs(80) if sp.bn})
BN_BAR = 1e-5          # elementwise fp32 ops on O(1) values with per-channel sums in fp64: a few ulp of the largest term


@pytest.mark.parametrize("C", BN_C)
@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
def test_bn_kernels(C, train):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    g = torch.Generator().manual_seed(C * 2 + train)
    P = 2 * 13 * 13 + 7
    z64 = (torch.randn(P, C, generator=g, dtype=torch.float64) * 3 + 1).float().double()
    res64 = torch.randn(P, C, generator=g, dtype=torch.float64).float().double()
    dy64 = torch.randn(P, C, generator=g, dtype=torch.float64).float().double()
    gam = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).float().double()
    bet = (torch.rand(C, generator=g, dtype=torch.float64) - 0.5).float().double()
    rm = torch.randn(C, generator=g, dtype=torch.float64).float().double()
    rv = (torch.rand(C, generator=g, dtype=torch.float64) * 4 + 0.1).float().double()
    d = {k: v.float().contiguous().to(DEV) for k, v in dict(z=z64, res=res64, dy=dy64, gam=gam, bet=bet, rm=rm, rv=rv).items()}
    mean, invstd, rmo, rvo = _buf(C), _buf(C), _buf(C), _buf(C)
    nb = lib.yv3_train_channel_workspace_bytes(P, C)
    ws = torch.empty(nb, device=DEV, dtype=torch.uint8)
    if train:
        assert lib.yv3_train_bn_stats(d["z"].data_ptr(), P, C, 1e-5, 0.1, d["rm"].data_ptr(), d["rv"].data_ptr(), rmo.data_ptr(),
                                      rvo.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), nb - 1, s) == _ffi.EWORKSPACE
        _ffi.check(lib.yv3_train_bn_stats(d["z"].data_ptr(), P, C, 1e-5, 0.1, d["rm"].data_ptr(), d["rv"].data_ptr(), rmo.data_ptr(),
                                          rvo.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), nb, s))
    else:
        _ffi.check(lib.yv3_train_bn_eval_stats(d["rm"].data_ptr(), d["rv"].data_ptr(), 1e-5, mean.data_ptr(), invstd.data_ptr(), C, s))
    y, dz, dgam, dbet = _buf(P * C), _buf(P * C), _buf(C), _buf(C)
    _ffi.check(lib.yv3_train_bn_act_fwd(d["z"].data_ptr(), mean.data_ptr(), invstd.data_ptr(), d["gam"].data_ptr(), d["bet"].data_ptr(),
                                        d["res"].data_ptr(), y.data_ptr(), P, C, s))
    _ffi.check(lib.yv3_train_bn_act_bwd(d["z"].data_ptr(), d["dy"].data_ptr(), mean.data_ptr(), invstd.data_ptr(), d["gam"].data_ptr(),
                                        d["bet"].data_ptr(), dz.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), P, C, train,
                                        ws.data_ptr(), nb, s))
    torch.cuda.synchronize()
    for b, n in ((mean, C), (invstd, C), (y, P * C), (dz, P * C), (dgam, C), (dbet, C)):
        assert _canary_ok(b, n)
    zz = z64.clone().requires_grad_(True)
    ga, be = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    rm2, rv2 = rm.clone(), rv.clone()
    u = F.batch_norm(zz.t().unsqueeze(0), rm2, rv2, ga, be, training=bool(train), momentum=0.1, eps=1e-5)
    y64 = F.leaky_relu(u, 0.1)[0].t() + res64
    y64.backward(dy64)

    def rel(got, ref):
        return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)

    assert rel(y[:P * C].view(P, C), y64.detach()) <= BN_BAR
    assert rel(dz[:P * C].view(P, C), zz.grad) <= BN_BAR
    assert rel(dgam[:C], ga.grad) <= BN_BAR and rel(dbet[:C], be.grad) <= BN_BAR
    if train:
        assert rel(rmo[:C], rm2) <= BN_BAR and rel(rvo[:C], rv2) <= BN_BAR


def test_error_codes():
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    t = torch.zeros(4096, device=DEV)
    p = t.data_ptr()
    assert lib.yv3_train_conv_fwd(None, None, p, None, p, 1, 8, 8, 32, 0, 32, 3, 1, 0, s) == _ffi.EINVAL
    assert lib.yv3_train_conv_fwd(p, None, p, None, p, 1, 8, 8, 32, 0, 32, 5, 1, 0, s) == _ffi.ESHAPE
    assert lib.yv3_train_conv_fwd(p, None, p, None, p, 1, 8, 8, 32, 0, 32, 3, 3, 0, s) == _ffi.ESHAPE
    assert lib.yv3_train_conv_fwd(p, None, p, None, p, 1, 8, 8, 32, 16, 32, 1, 1, 0, s) == _ffi.EINVAL      # cin_up without x2
    assert lib.yv3_train_conv_fwd(p, p, p, None, p, 1, 7, 8, 32, 16, 32, 1, 1, 0, s) == _ffi.ESHAPE         # odd H with cin_up
    assert lib.yv3_train_conv_dgrad(p, p, p, 0, 8, 8, 32, 32, 3, 1, 0, s) == _ffi.EINVAL
    assert lib.yv3_train_conv_wgrad_workspace_bytes(1, 8, 8, 32, 32, 2, 1) == 0
    assert lib.yv3_train_channel_workspace_bytes(0, 32) == 0
    assert lib.yv3_train_bn_act_bwd(p, p, p, p, p, p, p, p, None, 8, 8, 1, p, 1 << 20, s) == _ffi.EINVAL
    assert lib.yv3_train_upcat_bwd(p, p, p, 1, 7, 8, 8, 8, 0, 0, s) == _ffi.ESHAPE
    assert lib.yv3_train_pack_weight(p, None, None, 8, 8, 3, s) == _ffi.EINVAL
