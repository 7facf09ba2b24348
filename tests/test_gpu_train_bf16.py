"""The BF16 training step (net.backprop_math = BF16; yolo_v3_amd/backprop.py, csrc/train_bf16.hip) against the float64 restatement
tests/train_ref_bf16.py, plus the new C-ABI (cast, bf16 weight pack, bf16 conv forward / dgrad / wgrad) one layer shape at a time.

Precision bars.  The kernels round both operands to bf16 and accumulate in fp32; a product of two bf16 values is exact in fp32, so
against float64 over the *rounded* operands the error is the fp32 accumulation's alone, and the fp32 chain's bar of
tests/test_gpu_train.py applies per element.  A kernel that fed the unrounded fp32 operands misses that bar by orders of magnitude
(bf16 keeps 8 bits).  Whole steps compare every gradient and running statistic by relative L2 against the rounded float64 step, with
the bar BAR_FACTOR times the worst per-tensor error of the same rounded step run by torch in fp32 on the CPU (as test_gpu_train.py)."""
import copy
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_train_host as H
from tests import train_ref_bf16 as TB
from tests import yolo_loss_ref as R
from tests.helpers import trained_like_stream
from tests.test_gpu_train import SHAPES
from yolo_v3_amd import YoloNet, WeightManager, _ffi, synth, F32, BF16, F32X3, F32H2, Yv3Error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR_FACTOR = 16.0
CONV_BAR = 2e-6        # |got - ref| <= CONV_BAR * sum|a b|, ref over the bf16-rounded operands (fp32 accumulation only)
CANARY = 64


def make_net(size, C, math=BF16):
    net = YoloNet((size, size), numClass=C)
    WeightManager(net).load_stream(trained_like_stream(C))
    net = net.to(DEV)
    net.backprop, net.backprop_math = True, math
    return net


def gpu_step(net, x, tg):
    for p in net.parameters():
        p.grad = None
    loss = net(x.to(DEV), torch.as_tensor(tg))
    loss.backward()
    torch.cuda.synchronize()
    return loss


def pick_target(logits, size, C, B, T_rows, seed):
    for attempt in range(100):
        tg = R.random_rows(seed * 1000 + attempt, B, T_rows, C, (0.03, 0.8), n_valid_lo=3)
        res = TB.head_losses(logits, tg, size, C)
        if all(R.margins_ok(r["margins"]) for r in res) and sum(r["nGT"] for r in res) > 0:
            return tg
    raise AssertionError("no target draw clears the margins")


def check_against_ref(sd, net, loss, x, tg, C, train):
    ref = TB.run(sd, x, tg, C, train=train)
    ref32 = TB.run(sd, x, tg, C, train=train, dtype=torch.float32)
    # nCorrect counts predictions whose IoU clears 0.5: on logits that carry bf16 noise one such decision may go the other way
    assert net.stats["nGT"] == ref["stats"][8] and abs(net.stats["nCorrect"] - ref["stats"][7]) <= 1
    # (the loss sits behind 75 layers of bf16-rounded products: one fp32 difference upstream moves a rounding by 2^-9, so the loss is
    # held to the same bar as the gradients)
    worst = [("loss", abs(float(loss.detach()) - ref["loss"]) / abs(ref["loss"]), abs(ref32["loss"] - ref["loss"]) / abs(ref["loss"]))]
    named = dict(net.named_parameters())
    for k, g64 in ref["grads"].items():
        g = named[k].grad
        assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all(), k
        worst.append((k, TB.rel_l2(g.cpu(), g64), TB.rel_l2(ref32["grads"][k], g64)))
    mods = dict(net.named_modules())
    for prefix, (m64, v64) in ref["running"].items():
        bn = mods[prefix].bn
        worst.append((prefix + ".running_mean", TB.rel_l2(bn.running_mean.cpu(), m64), TB.rel_l2(ref32["running"][prefix][0], m64)))
        worst.append((prefix + ".running_var", TB.rel_l2(bn.running_var.cpu(), v64), TB.rel_l2(ref32["running"][prefix][1], v64)))
    bar = BAR_FACTOR * max(e32 for _, _, e32 in worst)
    worst.sort(key=lambda t: -t[1])
    print("bar %.3g; largest GPU errors (tensor, GPU, fp32 CPU):" % bar, [(k, "%.3g" % e, "%.3g" % e32) for k, e, e32 in worst[:4]])
    assert worst[0][1] <= bar, (bar, worst[:4])


# ---------------------------------------------------------------- cast
def test_cast_matches_torch_bfloat16():
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    u = []
    for e in (-149, -140, -127, -126, -100, -1, 0, 1, 20, 127):
        base = 2.0 ** e
        for m in (1.0, 1.25, 1.9921875, 1.99609375):               # (1.99609375 = the last bf16 step's halfway point: rounds up)
            u.append(base * m)
    bits = torch.tensor([0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x3f818001, 0x3f817fff,   # ties to even, just below / above
                         0x00008000, 0x00018000, 0x00007fff, 0x00008001, 0x007fffff, 0x00000001,   # subnormals and their ties
                         0x7f7fffff, 0x7f7f8000, 0x7f7f7fff, 0x80000000, 0x00000000, 0x7f800000, 0xff800000],
                        dtype=torch.int64).to(torch.int32)
    v = torch.cat([torch.tensor(u, dtype=torch.float32), -torch.tensor(u, dtype=torch.float32), bits.view(torch.float32),
                   -bits.view(torch.float32), torch.randn(4000, generator=torch.Generator().manual_seed(3)) * 1e3])
    v = torch.cat([v, torch.tensor([float("nan"), -float("nan")])])
    n = v.numel()
    src = v.to(DEV)
    dst = torch.full((n + CANARY,), 0x1234, device=DEV, dtype=torch.int16)
    _ffi.check(lib.yv3_train_to_bf16(src.data_ptr(), dst.data_ptr(), n, 1, 1, s))
    torch.cuda.synchronize()
    assert bool((dst[n:] == 0x1234).all())
    got = dst[:n].cpu()
    want = src.to(torch.bfloat16).view(torch.int16).cpu()
    nan = torch.isnan(v)
    assert torch.equal(got[~nan], want[~nan]), v[~nan][got[~nan] != want[~nan]][:8]
    assert bool(torch.isnan(got[nan].view(torch.bfloat16)).all())
    # the padded form: rows of C fp32 -> rows of ld bf16, zero channels appended
    P, C, ld = 37, 255, 256
    a = torch.randn(P, C, device=DEV)
    d = torch.full((P * ld + CANARY,), 0x1234, device=DEV, dtype=torch.int16)
    _ffi.check(lib.yv3_train_to_bf16(a.data_ptr(), d.data_ptr(), P, C, ld, s))
    torch.cuda.synchronize()
    assert bool((d[P * ld:] == 0x1234).all())
    dd = d[:P * ld].view(P, ld)
    assert torch.equal(dd[:, :C], a.to(torch.bfloat16).view(torch.int16)) and bool((dd[:, C:] == 0).all())


# ---------------------------------------------------------------- conv kernels, one distinct layer shape at a time
def _buf(n):
    return torch.full((n + CANARY,), float("nan"), device=DEV, dtype=torch.float32)


def _canary_ok(b, n):
    return bool(torch.isnan(b[n:]).all())


def _close(got, ref, scale, what):
    assert torch.isfinite(got).all(), what + ": non-finite"
    worst = float(((got.double().cpu() - ref).abs() / (scale + 1e-30)).max())
    assert worst <= CONV_BAR, "%s: %.3g > %.3g" % (what, worst, CONV_BAR)


def _r8(c):
    return (c + 7) // 8 * 8


@pytest.mark.parametrize("sh", SHAPES, ids=[s["name"] for s in SHAPES])
def test_conv_kernels_per_shape(sh):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    B, H, cin, cout, k, st, cu = 2, sh["H"], sh["cin"], sh["cout"], sh["k"], sh["stride"], sh["cin_up"]
    W, nchw, cp = H, int(cin == 3), _r8(cout)
    g = torch.Generator().manual_seed(zlib.crc32(sh["name"].encode()) + 1)
    pad = (k - 1) // 2
    x32 = torch.randn(B, cin, H, W, generator=g)
    w32 = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
    if cu:
        low = torch.randn(B, cu, H // 2, W // 2, generator=g)
        x32[:, :cu] = F.interpolate(low, scale_factor=2, mode="nearest")
        xin = TB.rb(x32[:, cu:]).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
        x2 = TB.rb(low).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
    else:
        xin = (x32 if nchw else x32.permute(0, 2, 3, 1)).contiguous().to(torch.bfloat16).to(DEV)
        x2 = None
    x2p = x2.data_ptr() if x2 is not None else None
    x64, w64 = TB.rb(x32).double(), TB.rb(w32).double()
    # weight images (from the fp32 weight: the pack rounds), with canaries past both
    wd32 = w32.contiguous().to(DEV)
    nwp = cp * cin * k * k
    wf = torch.full((nwp + CANARY,), 0x1234, device=DEV, dtype=torch.int16)
    wdd = torch.full((nwp + CANARY,), 0x1234, device=DEV, dtype=torch.int16)
    _ffi.check(lib.yv3_train_pack_weight_bf16(wd32.data_ptr(), wf.data_ptr(), wdd.data_ptr(), cout, cin, k, s))
    torch.cuda.synchronize()
    assert bool((wf[nwp:] == 0x1234).all()) and bool((wdd[nwp:] == 0x1234).all())
    wfv = wf[:nwp].view(cp, k * k, cin)                    # [n][tap][ci]
    ref_wf = torch.zeros(cp, k * k, cin, dtype=torch.bfloat16)
    ref_wf[:cout] = w32.permute(0, 2, 3, 1).reshape(cout, k * k, cin).to(torch.bfloat16)
    assert torch.equal(wfv.cpu(), ref_wf.view(torch.int16))
    # forward
    z64 = F.conv2d(x64, w64, stride=st, padding=pad)
    za = F.conv2d(x64.abs(), w64.abs(), stride=st, padding=pad)
    Ho = z64.shape[2]
    nz = B * Ho * Ho * cout
    z = _buf(nz)
    _ffi.check(lib.yv3_train_conv_fwd_bf16(xin.data_ptr(), x2p, wf.data_ptr(), None, z.data_ptr(), B, H, W, cin, cu, cout, k, st,
                                           nchw, s))
    torch.cuda.synchronize()
    assert _canary_ok(z, nz)
    _close(z[:nz].view(B, Ho, Ho, cout), z64.permute(0, 2, 3, 1), za.permute(0, 2, 3, 1), "fwd")
    # dz: bf16, coutp channels, the padding zero
    dz32 = torch.randn(B, cout, Ho, Ho, generator=g)
    dz64 = TB.rb(dz32).double()
    dzp = torch.zeros(B, Ho, Ho, cp, dtype=torch.bfloat16)
    dzp[..., :cout] = dz32.permute(0, 2, 3, 1).to(torch.bfloat16)
    dzd = dzp.contiguous().to(DEV)
    if not nchw:
        nx = B * H * W * cin
        for acc in (0, 1):
            dx = _buf(nx)
            base = torch.randn(nx, generator=g).to(DEV)
            if acc:
                dx[:nx] = base
            _ffi.check(lib.yv3_train_conv_dgrad_bf16(dzd.data_ptr(), wdd.data_ptr(), dx.data_ptr(), B, H, W, cin, cout, k, st, acc, s))
            torch.cuda.synchronize()
            assert _canary_ok(dx, nx)
            ref = torch.nn.grad.conv2d_input(x64.shape, w64, dz64, stride=st, padding=pad).permute(0, 2, 3, 1)
            sc = torch.nn.grad.conv2d_input(x64.shape, w64.abs(), dz64.abs(), stride=st, padding=pad).permute(0, 2, 3, 1)
            if acc:
                ref = ref + base.cpu().double().view(B, H, W, cin)
                sc = sc + base.cpu().double().abs().view(B, H, W, cin)
            _close(dx[:nx].view(B, H, W, cin), ref, sc, "dgrad acc=%d" % acc)
    nb = lib.yv3_train_conv_wgrad_bf16_workspace_bytes(B, H, W, cin, cout, k, st)
    assert nb > 0
    ws = torch.empty(nb, device=DEV, dtype=torch.uint8)
    nw = cout * cin * k * k
    dw = _buf(nw)
    assert lib.yv3_train_conv_wgrad_bf16(xin.data_ptr(), x2p, dzd.data_ptr(), dw.data_ptr(), B, H, W, cin, cu, cout, k, st, nchw,
                                         ws.data_ptr(), nb - 1, s) == _ffi.EWORKSPACE
    _ffi.check(lib.yv3_train_conv_wgrad_bf16(xin.data_ptr(), x2p, dzd.data_ptr(), dw.data_ptr(), B, H, W, cin, cu, cout, k, st, nchw,
                                             ws.data_ptr(), nb, s))
    torch.cuda.synchronize()
    assert _canary_ok(dw, nw)
    ref = torch.nn.grad.conv2d_weight(x64, w64.shape, dz64, stride=st, padding=pad)
    sc = torch.nn.grad.conv2d_weight(x64.abs(), w64.shape, dz64.abs(), stride=st, padding=pad)
    _close(dw[:nw].view(cout, cin, k, k), ref, sc, "wgrad")


def test_error_codes():
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    t = torch.zeros(1 << 16, device=DEV)
    p = t.data_ptr()
    E, S, WS = _ffi.EINVAL, _ffi.ESHAPE, _ffi.EWORKSPACE
    assert lib.yv3_train_to_bf16(None, p, 8, 8, 8, s) == E
    assert lib.yv3_train_to_bf16(p, None, 8, 8, 8, s) == E
    assert lib.yv3_train_to_bf16(p, p, 0, 8, 8, s) == E
    assert lib.yv3_train_to_bf16(p, p, 8, 8, 7, s) == E                       # ld < C
    assert lib.yv3_train_pack_weight_bf16(None, p, p, 8, 8, 3, s) == E
    assert lib.yv3_train_pack_weight_bf16(p, None, None, 8, 8, 3, s) == E
    assert lib.yv3_train_pack_weight_bf16(p, p, None, 0, 8, 3, s) == E
    assert lib.yv3_train_pack_weight_bf16(p, p, None, 8, 8, 5, s) == S
    assert lib.yv3_train_conv_fwd_bf16(None, None, p, None, p, 1, 8, 8, 32, 0, 32, 3, 1, 0, s) == E
    assert lib.yv3_train_conv_fwd_bf16(p, None, None, None, p, 1, 8, 8, 32, 0, 32, 3, 1, 0, s) == E
    assert lib.yv3_train_conv_fwd_bf16(p, None, p, None, None, 1, 8, 8, 32, 0, 32, 3, 1, 0, s) == E
    assert lib.yv3_train_conv_fwd_bf16(p, None, p, None, p, 0, 8, 8, 32, 0, 32, 3, 1, 0, s) == E
    assert lib.yv3_train_conv_fwd_bf16(p, None, p, None, p, 1, 8, 8, 32, 0, 32, 5, 1, 0, s) == S
    assert lib.yv3_train_conv_fwd_bf16(p, None, p, None, p, 1, 8, 8, 32, 0, 32, 3, 3, 0, s) == S
    assert lib.yv3_train_conv_fwd_bf16(p, None, p, None, p, 1, 8, 8, 36, 0, 32, 3, 1, 0, s) == S     # NHWC cin % 8 != 0
    assert lib.yv3_train_conv_fwd_bf16(p, p, p, None, p, 1, 8, 8, 32, 12, 32, 1, 1, 0, s) == S       # cin_up % 8 != 0
    assert lib.yv3_train_conv_fwd_bf16(p, None, p, None, p, 1, 8, 8, 32, 16, 32, 1, 1, 0, s) == E    # cin_up without x2
    assert lib.yv3_train_conv_fwd_bf16(p, p, p, None, p, 1, 7, 8, 32, 16, 32, 1, 1, 0, s) == S       # odd H with cin_up
    assert lib.yv3_train_conv_fwd_bf16(p, p, p, None, p, 1, 8, 8, 32, 16, 32, 1, 1, 1, s) == S       # NCHW with cin_up
    assert lib.yv3_train_conv_dgrad_bf16(None, p, p, 1, 8, 8, 32, 32, 3, 1, 0, s) == E
    assert lib.yv3_train_conv_dgrad_bf16(p, None, p, 1, 8, 8, 32, 32, 3, 1, 0, s) == E
    assert lib.yv3_train_conv_dgrad_bf16(p, p, None, 1, 8, 8, 32, 32, 3, 1, 0, s) == E
    assert lib.yv3_train_conv_dgrad_bf16(p, p, p, 0, 8, 8, 32, 32, 3, 1, 0, s) == E
    assert lib.yv3_train_conv_dgrad_bf16(p, p, p, 1, 8, 8, 32, 32, 2, 1, 0, s) == S
    assert lib.yv3_train_conv_wgrad_bf16_workspace_bytes(1, 8, 8, 32, 32, 2, 1) == 0
    assert lib.yv3_train_conv_wgrad_bf16_workspace_bytes(1, 8, 8, 32, 32, 3, 4) == 0
    nb = lib.yv3_train_conv_wgrad_bf16_workspace_bytes(1, 8, 8, 32, 32, 3, 1)
    assert 0 < nb <= 4 * t.numel()
    assert lib.yv3_train_conv_wgrad_bf16(None, None, p, p, 1, 8, 8, 32, 0, 32, 3, 1, 0, p, nb, s) == E
    assert lib.yv3_train_conv_wgrad_bf16(p, None, None, p, 1, 8, 8, 32, 0, 32, 3, 1, 0, p, nb, s) == E
    assert lib.yv3_train_conv_wgrad_bf16(p, None, p, None, 1, 8, 8, 32, 0, 32, 3, 1, 0, p, nb, s) == E
    assert lib.yv3_train_conv_wgrad_bf16(p, None, p, p, 1, 8, 8, 32, 0, 32, 3, 1, 0, None, nb, s) == E
    assert lib.yv3_train_conv_wgrad_bf16(p, None, p, p, 1, 8, 8, 32, 16, 32, 3, 1, 0, p, nb, s) == E    # cin_up without x2
    assert lib.yv3_train_conv_wgrad_bf16(p, None, p, p, 1, 8, 8, 32, 0, 32, 5, 1, 0, p, nb, s) == S
    assert lib.yv3_train_conv_wgrad_bf16(p, None, p, p, 1, 8, 8, 36, 0, 32, 3, 1, 0, p, 1 << 20, s) == S
    assert lib.yv3_train_conv_wgrad_bf16(p, None, p, p, 1, 8, 8, 32, 0, 32, 3, 1, 0, p, nb - 1, s) == WS
    torch.cuda.synchronize()


# ---------------------------------------------------------------- whole step against the rounded float64 step
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_fixture_step_matches_float64(train):
    sd, x, tg, _ = H.case()
    C, size = H.CASE["C"], H.CASE["size"]
    net = make_net(size, C)
    net.train(train)
    x = torch.from_numpy(x)
    loss = gpu_step(net, x, tg)
    assert loss.requires_grad
    check_against_ref(sd, net, loss, x, tg, C, train)
    assert int(net.feature.mlist[0].bn.num_batches_tracked) == (1 if train else 0)


def test_416_step_matches_float64():
    C, size, B = 80, 416, 4
    net = make_net(size, C).train()
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = torch.from_numpy(synth.images(B, size, 511))
    logits, _, _ = TB.forward(sd, x, True)
    tg = pick_target(logits, size, C, B, 20, 43)
    loss = gpu_step(net, x, tg)
    check_against_ref(sd, net, loss, x, tg, C, True)


# ---------------------------------------------------------------- semantics
def _small_case(train=True, math=BF16):
    C, size, B = 3, 96, 2
    net = make_net(size, C, math).train(train)
    x = torch.from_numpy(synth.images(B, size, 31))
    tg = R.random_rows(77, B, 8, C, (0.05, 0.7))
    return net, x, tg


def _grads(net):
    return {k: (p.grad.clone() if p.grad is not None else None) for k, p in net.named_parameters()}


def test_bf16_steps_are_bitwise_deterministic():
    net, x, tg = _small_case()
    a, b = copy.deepcopy(net), copy.deepcopy(net)
    la, lb = gpu_step(a, x, tg), gpu_step(b, x, tg)
    assert float(la) == float(lb)
    ga, gb = _grads(a), _grads(b)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for (k, t1), (_, t2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(t1, t2), k


def test_bf16_differs_from_f32_and_explicit_f32_is_the_default():
    net, x, tg = _small_case(math=F32)
    default = copy.deepcopy(net)
    del default.backprop_math                      # (the attribute's default, as a fresh YoloNet has it)
    fresh = YoloNet((96, 96), numClass=3)
    assert fresh.backprop_math == F32
    default.backprop_math = fresh.backprop_math
    bf = copy.deepcopy(net)
    bf.backprop_math = BF16
    l1, l2, l3 = gpu_step(net, x, tg), gpu_step(default, x, tg), gpu_step(bf, x, tg)
    assert float(l1) == float(l2)
    g1, g2, g3 = _grads(net), _grads(default), _grads(bf)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    assert any(not torch.equal(g1[k], g3[k]) for k in g1)


def test_frozen_backbone_stops_at_the_heads():
    net, x, tg = _small_case()
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


def test_sgd_reduces_the_loss():
    net, x, tg = _small_case()
    opt = torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = net(x.to(DEV), torch.as_tensor(tg))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1000)
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses
    assert all(p.dtype == torch.float32 for p in net.parameters())


def test_no_grad_bf16_loss_is_the_forward_of_the_step():
    net, x, tg = _small_case(train=False)
    a = copy.deepcopy(net)
    with torch.no_grad():
        l0 = net(x.to(DEV), torch.as_tensor(tg))
    assert not l0.requires_grad
    l1 = gpu_step(a, x, tg)
    assert float(l0) == float(l1)


@pytest.mark.parametrize("bad", ["F32X3", "F32H2", "garbage"])
def test_invalid_backprop_math_raises_before_any_launch(bad):
    net, x, tg = _small_case()
    net.backprop_math = {"F32X3": F32X3, "F32H2": F32H2}.get(bad, bad)
    before = copy.deepcopy(net.state_dict())
    xd, td = x.to(DEV), torch.as_tensor(tg)
    torch.cuda.synchronize()
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            with pytest.raises(Yv3Error) as e:
                net(xd, td)
        assert e.value.code == _ffi.EINVAL
    torch.cuda.synchronize()
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k                     # no BatchNorm statistic moved, num_batches_tracked included
    assert all(p.grad is None for p in net.parameters())
