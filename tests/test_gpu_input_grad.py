"""The training path as an autograd citizen (yolo_v3_amd/backprop.py, yolo_v3_amd/yololayer.py): net.logits(x), the opt-in input
gradient (net.input_grad; yv3_train_conv0_dgrad[_bf16]) and the differentiable decode (yv3_decode_bwd_nchw), against the float64
restatements tests/train_ref.py, tests/train_ref_bf16.py (run with a leaf x), tests/train_kernel_ref.py and tests/decode_ref.py.

Precision bars (the project's existing ones).  Whole-step tensors -- every parameter gradient and x.grad -- are compared by relative
L2 against float64 with one bar per case: BAR_FACTOR times the largest such error torch fp32 on the CPU shows on the same case.  The
layer-0 dgrad kernels are held per element to |got - ref| <= CONV_BAR * sum|a b| (BF16: over the bf16-rounded operands, whose
products are exact in fp32).  The decode backward is held per element: |got - ref| / (|dout| S), S the scale of the derivative
(tests/decode_ref.decode_grad), at most BAR_FACTOR times the largest such error of torch fp32 CPU autograd over the same formula."""
import copy
import functools

import pytest
import torch

from tests import decode_ref as D
from tests import test_input_grad_host as HG
from tests import train_kernel_ref as K
from tests import train_ref as T
from tests import train_ref_bf16 as TB
from tests import yolo_loss_ref as R
from tests.helpers import trained_like_stream
from yolo_v3_amd import YoloNet, YoloLayer, WeightManager, _ffi, arch, synth, F32, BF16, F32X3, Yv3Error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR_FACTOR = 16.0
CONV_BAR = K.CONV_BAR
CANARY = 64
SIZE, C, B = 96, 3, 2
MATHS = pytest.mark.parametrize("math", [F32, BF16], ids=["f32", "bf16"])


# ---------------------------------------------------------------- the shared case and its references (computed once)
@functools.lru_cache(maxsize=None)
def base_net():
    net = YoloNet((SIZE, SIZE), numClass=C)
    WeightManager(net).load_stream(trained_like_stream(C))
    return net.to(DEV)


def make_net(train=True, math=F32, input_grad=True):
    net = copy.deepcopy(base_net()).train(train)
    net.backprop, net.backprop_math, net.input_grad = True, math, input_grad
    return net


@functools.lru_cache(maxsize=None)
def case():
    """(state_dict on the CPU, images, target) -- _fixture_case of tests/test_gpu_train.py."""
    sd = {k: v.detach().cpu().clone() for k, v in base_net().state_dict().items()}
    return sd, torch.from_numpy(synth.images(B, SIZE, 31)), R.random_rows(77, B, 8, C, (0.05, 0.7))


def ref_forward(train, math, dtype):
    """-> (leaf x, (logits, leaf parameters, running statistics)) of the float64 / fp32 CPU restatement."""
    sd, x, _ = case()
    xl = x.to(dtype).clone().requires_grad_(True)
    return xl, (TB.forward if math == BF16 else T.forward)(sd, xl, train, dtype)


def grads_of(xl, P):
    out = {k: (p.grad.detach() if p.grad is not None else None) for k, p in P.items()}
    out["x"] = xl.grad.detach()
    return out


@functools.lru_cache(maxsize=None)
def ref_step(train, math):
    """The YOLO-loss step with a leaf x -> {dtype: dict(loss, grads incl. "x")} for float64 and the fp32 yardstick."""
    sd, x, tg = case()
    out = {}
    for dtype in (torch.float64, torch.float32):
        xl, fw = ref_forward(train, math, dtype)
        r = T.run(sd, xl, tg, C, train=train, dtype=dtype, logits_and_params=fw)
        out[dtype] = dict(loss=r["loss"], grads=dict(r["grads"], x=xl.grad.detach()))
    return out


def check_grads(net, xgrad, ref64, ref32, what):
    """Every parameter gradient of net and xgrad against ref64 at the whole-step bar (yardstick: ref32)."""
    named = dict(net.named_parameters())
    rows = []
    for k, g64 in ref64.items():
        g = xgrad if k == "x" else named[k].grad
        if g64 is None:
            assert g is None, k
            continue
        assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all(), k
        rows.append((k, T.rel_l2(g.cpu(), g64), T.rel_l2(ref32[k], g64)))
    bar = BAR_FACTOR * max(e32 for _, _, e32 in rows)
    rows.sort(key=lambda t: -t[1])
    print("%s: bar %.3g; x.grad %.3g; largest GPU errors (tensor, GPU, fp32 CPU):" % (what, bar, dict((k, e) for k, e, _ in rows)["x"]),
          [(k, "%.3g" % e, "%.3g" % e32) for k, e, e32 in rows[:4]])
    assert rows[0][1] <= bar, (bar, rows[:4])


def param_grads(net):
    return {k: (p.grad.clone() if p.grad is not None else None) for k, p in net.named_parameters()}


def assert_same_grads_and_state(a, b):
    ga, gb = param_grads(a), param_grads(b)
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None) and (ga[k] is None or torch.equal(ga[k], gb[k])), k
    for (k, t1), (_, t2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(t1, t2), k


# ---------------------------------------------------------------- 1. the layer-0 dgrad kernels through the C-ABI
DGRAD_SHAPES = [(1, 1, 1, 32), (1, 3, 5, 32), (2, 33, 70, 32), (2, 32, 96, 32), (1, 416, 416, 32), (1, 5, 67, 72)]


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", DGRAD_SHAPES, ids=["x".join(map(str, s)) for s in DGRAD_SHAPES])
def test_conv0_dgrad_kernel(shape, bf):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    b, H, W, cout = shape
    coutp = (cout + 7) // 8 * 8
    g = torch.Generator().manual_seed(H * 1000 + W + int(bf))
    dz32 = torch.randn(b, cout, H, W, generator=g)
    w32 = torch.randn(cout, 3, 3, 3, generator=g) / 27 ** 0.5
    if bf:
        dz64, w64 = K.rb(dz32).double(), K.rb(w32).double()
        dzp = torch.zeros(b, H, W, coutp, dtype=torch.bfloat16)
        dzp[..., :cout] = dz32.permute(0, 2, 3, 1).to(torch.bfloat16)
        dzd, fn = dzp.contiguous().to(DEV), lib.yv3_train_conv0_dgrad_bf16
    else:
        dz64, w64 = dz32.double(), w32.double()
        dzd, fn = dz32.permute(0, 2, 3, 1).contiguous().to(DEV), lib.yv3_train_conv0_dgrad
    wd = w32.contiguous().to(DEV)                                     # (the fp32 parameter itself: the bf16 kernel rounds it)
    ref, scale = K.conv_dgrad((b, 3, H, W), w64, dz64, 1)
    n = b * 3 * H * W
    outs = []
    for _ in range(2):
        dx = torch.full((n + CANARY,), float("nan"), device=DEV, dtype=torch.float32)
        _ffi.check(fn(dzd.data_ptr(), wd.data_ptr(), dx.data_ptr(), b, H, W, cout, s))
        torch.cuda.synchronize()
        assert bool(torch.isnan(dx[n:]).all()), "canary"
        assert bool(torch.isfinite(dx[:n]).all())
        outs.append(dx[:n].view(b, 3, H, W))
    assert torch.equal(outs[0], outs[1])
    worst = K.conv_ratio(outs[0], ref, scale)
    print("worst |got - ref| / (CONV_BAR sum|a b|) = %.3g" % worst)
    assert worst <= 1.0


def test_conv0_dgrad_bad_arguments():
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    t = torch.zeros(4096, device=DEV)
    p = t.data_ptr()
    E, S = _ffi.EINVAL, _ffi.ESHAPE
    for fn in (lib.yv3_train_conv0_dgrad, lib.yv3_train_conv0_dgrad_bf16):
        assert fn(None, p, p, 1, 4, 4, 32, s) == E
        assert fn(p, None, p, 1, 4, 4, 32, s) == E
        assert fn(p, p, None, 1, 4, 4, 32, s) == E
        assert fn(p, p, p, 0, 4, 4, 32, s) == E
        assert fn(p, p, p, 1, 0, 4, 32, s) == E
        assert fn(p, p, p, 1, 4, -1, 32, s) == E
        assert fn(p, p, p, 1, 4, 4, 0, s) == E
        assert fn(p, p, p, 1 << 20, 1 << 14, 1 << 14, 32, s) == S      # more tiles than an int counts
    assert lib.yv3_train_conv0_dgrad(p, p, p, 1, 4, 4, 30, s) == S     # fp32 dz rows must stay 16-byte aligned
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. a whole step with net.input_grad = True
@MATHS
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_step_with_input_grad_matches_float64(train, math):
    _, x, tg = case()
    tgt = torch.as_tensor(tg)
    net, plain = make_net(train, math), make_net(train, math, input_grad=False)
    xg = x.to(DEV).requires_grad_(True)
    loss = net(xg, tgt)
    assert loss.requires_grad
    loss.backward()
    loss_plain = plain(x.to(DEV), tgt)
    loss_plain.backward()
    torch.cuda.synchronize()
    assert xg.grad is not None and xg.grad.shape == xg.shape and xg.grad.dtype == xg.dtype
    ref = ref_step(train, math)
    check_grads(net, xg.grad, ref[torch.float64]["grads"], ref[torch.float32]["grads"], "step")
    # asking for x.grad changes nothing else: loss, parameter gradients and running statistics are the plain step's bits
    assert float(loss.detach()) == float(loss_plain.detach())
    assert_same_grads_and_state(net, plain)
    # a second backward into the same x accumulates (the forward does not depend on the running statistics that moved)
    g1 = xg.grad.clone()
    net(xg, tgt).backward()
    torch.cuda.synchronize()
    assert torch.equal(xg.grad, g1 + g1)


# ---------------------------------------------------------------- 3. arbitrary upstream gradients through net.logits
@functools.lru_cache(maxsize=None)
def ref_upstream(math, only_last):
    out = {}
    for dtype in (torch.float64, torch.float32):
        xl, (logits, P, _) = ref_forward(True, math, dtype)
        Rk = [r.float().to(dtype) for r in HG.upstream(logits, 11)]
        if only_last:
            torch.autograd.backward(logits[2:], Rk[2:])
        else:
            torch.autograd.backward(logits, Rk)
        out[dtype] = grads_of(xl, P)
    return out, [r.float() for r in Rk]


@MATHS
@pytest.mark.parametrize("only_last", [False, True], ids=["three_heads", "lg3_only"])
def test_arbitrary_upstream_gradients(only_last, math):
    _, x, _ = case()
    ref, Rk = ref_upstream(math, only_last)
    net = make_net(True, math)
    xg = x.to(DEV).requires_grad_(True)
    lg = net.logits(xg)
    assert all(l.requires_grad for l in lg) and [tuple(l.shape) for l in lg] == [tuple(r.shape) for r in Rk]
    Rd = [r.to(DEV) for r in Rk]
    # head 1: the product in NHWC (the gradient arrives with the logits' own strides); head 2: transposed (arrives with neither
    # layout's strides); head 3: a plain NCHW tensor
    terms = [(lg[0].permute(0, 2, 3, 1) * Rd[0].permute(0, 2, 3, 1).contiguous()).sum(),
             (lg[1].transpose(2, 3) * Rd[1].transpose(2, 3).contiguous()).sum(),
             (lg[2] * Rd[2]).sum()]
    L = terms[2] if only_last else terms[0] + terms[1] + terms[2]
    L.backward()
    torch.cuda.synchronize()
    check_grads(net, xg.grad, ref[torch.float64], ref[torch.float32], "upstream")
    if only_last:                                     # the other heads' own convolutions received nothing
        named = dict(net.named_parameters())
        for k in ("pre_det1.mlist.6.weight", "pre_det1.mlist.6.bias", "pre_det2.mlist.6.weight", "pre_det1.mlist.5.conv.weight"):
            assert named[k].grad is None, k


# ---------------------------------------------------------------- 4. the composite: YoloLayer losses on net.logits == net(x, target)
@MATHS
def test_yolo_layers_on_logits_are_the_training_step(math):
    _, x, tg = case()
    tgt = torch.as_tensor(tg)
    a, b = make_net(True, math, input_grad=False), make_net(True, math, input_grad=False)
    xd = x.to(DEV)
    lg = a.logits(xd)
    la = sum(head(l, a.img_dim, tgt)[0] for head, l in zip((a.yolo1, a.yolo2, a.yolo3), lg))
    la.backward()
    lb = b(xd, tgt)
    lb.backward()
    torch.cuda.synchronize()
    assert float(la.detach()) == float(lb.detach())
    assert all(p.grad is not None for p in a.parameters())
    assert_same_grads_and_state(a, b)


# ---------------------------------------------------------------- 5. saliency: everything frozen, eval mode
@MATHS
def test_saliency_with_frozen_parameters(math):
    _, x, tg = case()
    tgt = torch.as_tensor(tg)
    frozen, free = make_net(False, math), make_net(False, math)
    for p in frozen.parameters():
        p.requires_grad_(False)
    before = {k: v.clone() for k, v in frozen.state_dict().items()}
    xa, xb = x.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    la = frozen(xa, tgt)
    assert la.requires_grad
    la.backward()
    free(xb, tgt).backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in frozen.parameters())
    for k, v in frozen.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert xa.grad is not None and bool(xa.grad.abs().max() > 0) and torch.equal(xa.grad, xb.grad)


# ---------------------------------------------------------------- 6. modes and defaults
def test_logits_modes_and_defaults():
    _, x, _ = case()
    xd = x.to(DEV)
    net = make_net(True, F32, input_grad=False)
    net.backprop = False                              # (logits does not depend on it)
    nbt = lambda: int(net.feature.mlist[0].bn.num_batches_tracked)
    with torch.no_grad():
        lg = net.logits(xd)
    assert all(l.grad_fn is None and not l.requires_grad for l in lg) and nbt() == 1
    assert [tuple(l.shape) for l in lg] == [(B, 3 * (5 + C), SIZE // st, SIZE // st) for st in (32, 16, 8)]
    assert all(l.permute(0, 2, 3, 1).is_contiguous() and l.dtype == torch.float32 for l in lg)
    lg2 = net.logits(xd)
    assert all(l.grad_fn is not None for l in lg2) and nbt() == 2
    for u, v in zip(lg, lg2):                         # (train mode: the batch statistics, not the running ones, shape the output)
        assert torch.equal(u, v)
    net.eval()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.logits(xd)
    assert nbt() == 2
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    for p in net.parameters():
        p.requires_grad_(False)
    assert all(l.grad_fn is None for l in net.logits(xd))             # nothing requires grad: forward only
    assert net.input_grad is False and YoloNet((SIZE, SIZE), numClass=C).input_grad is False
    with pytest.raises(NotImplementedError):
        net.logits(xd.clone().requires_grad_(True))
    net.backprop_math = F32X3
    with pytest.raises(Yv3Error) as e:
        net.logits(xd)
    assert e.value.code == _ffi.EINVAL


# ---------------------------------------------------------------- 7. the differentiable decode
def decode_case(b, c, H, W, head, seed):
    g = torch.Generator().manual_seed(seed)
    lg = torch.rand(b, 3 * (5 + c), H, W, generator=g) * 8 - 4
    dout = torch.randn(b, H * W * 3, 5 + c, generator=g)
    return lg, dout, HG.ANCHORS[head], 32.0 / 2 ** head


def decode_error(got, lg, dout, anchors, stride):
    """-> (largest normalised error of got, of torch fp32 CPU autograd) against tests/decode_ref.decode_grad in float64."""
    ref, S = D.decode_grad(lg.double(), anchors, stride, dout.double())
    l32 = lg.clone().requires_grad_(True)
    D.decode(l32, anchors, stride).backward(dout)
    b, _, H, W = lg.shape
    norm = D._unrows(dout.double().reshape(b, H, W, 3, -1)).abs() * S + 1e-300
    return float(((got.double().cpu() - ref).abs() / norm).max()), float(((l32.grad.double() - ref).abs() / norm).max())


@pytest.mark.parametrize("b,c,H,W,head,noncontig", [(2, 3, 3, 5, 0, False), (1, 80, 13, 13, 0, False), (2, 3, 3, 5, 1, True)],
                         ids=["3x5", "13x13_c80", "3x5_noncontiguous_dout"])
def test_decode_backward(b, c, H, W, head, noncontig):
    lg, dout, anchors, stride = decode_case(b, c, H, W, head, 100 * H + c)
    pairs = [tuple(arch.DEFAULT_ANCHORS[i:i + 2]) for i in range(0, 18, 2)]
    layer = YoloLayer(pairs, list(arch.ANCHOR_MASKS[head]), (stride * W, stride * H), c)      # (net.yolo1 / yolo2 of such a net)
    img_dim = (stride * W, stride * H)
    ld = lg.to(DEV)
    with torch.no_grad():
        plain = layer(ld, img_dim)
    lreq = ld.clone().requires_grad_(True)
    out = layer(lreq, img_dim)
    assert out.grad_fn is not None and plain.grad_fn is None and torch.equal(out.detach(), plain)
    dd = dout.to(DEV)
    if noncontig:                                     # the gradient arrives as a transposed view
        (out.transpose(1, 2) * dd.transpose(1, 2).contiguous()).sum().backward()
    else:
        out.backward(dd)
    torch.cuda.synchronize()
    assert lreq.grad is not None and lreq.grad.shape == lreq.shape
    e, e32 = decode_error(lreq.grad, lg, dout, anchors, stride)
    print("decode backward: normalised error %.3g, torch fp32 CPU %.3g" % (e, e32))
    assert e32 > 0 and e <= BAR_FACTOR * e32


@functools.lru_cache(maxsize=None)
def ref_decoded():
    out = {}
    for dtype in (torch.float64, torch.float32):
        xl, (logits, P, _) = ref_forward(True, F32, dtype)
        dec = torch.cat([D.decode(l, HG.ANCHORS[k], 32.0 / 2 ** k) for k, l in enumerate(logits)], 1)
        Rm = torch.randn(dec.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64).float()
        (dec * Rm.to(dtype)).sum().backward()
        out[dtype] = grads_of(xl, P)
    return out, Rm


def test_decoded_boxes_train_the_net_end_to_end():
    _, x, _ = case()
    ref, Rm = ref_decoded()
    net = make_net(True, F32)
    xg = x.to(DEV).requires_grad_(True)
    lg = net.logits(xg)
    dec = torch.cat([head(l, net.img_dim) for head, l in zip((net.yolo1, net.yolo2, net.yolo3), lg)], 1)
    assert dec.grad_fn is not None and dec.shape == Rm.shape
    (dec * Rm.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    check_grads(net, xg.grad, ref[torch.float64], ref[torch.float32], "decode end to end")
