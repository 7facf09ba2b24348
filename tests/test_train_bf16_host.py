"""The BF16 training step's host side (CPU only): the float64 restatement tests/train_ref_bf16.py against tests/train_ref.py and
against autograd through explicit rounding, the default of net.backprop_math, and the ctypes prototypes of the new C-ABI."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import test_train_host as H
from tests import train_ref as T
from tests import train_ref_bf16 as TB
from yolo_v3_amd import _ffi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("yv3_train_to_bf16", "yv3_train_pack_weight_bf16", "yv3_train_conv_fwd_bf16", "yv3_train_conv_dgrad_bf16",
       "yv3_train_conv_wgrad_bf16_workspace_bytes", "yv3_train_conv_wgrad_bf16")


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_restatement_without_rounding_is_train_ref(train):
    sd, x, tg, _ = H.case()
    C = H.CASE["C"]
    a = T.run(sd, x, tg, C, train=train)
    b = TB.run(sd, x, tg, C, train=train, rounding=False)
    assert abs(a["loss"] - b["loss"]) <= 1e-12 * abs(a["loss"])
    assert a["stats"] == b["stats"]
    for k, g in a["grads"].items():
        assert T.rel_l2(b["grads"][k], g) <= 1e-12, k
    for k, (m, v) in a["running"].items():
        assert T.rel_l2(b["running"][k][0], m) <= 1e-12 and T.rel_l2(b["running"][k][1], v) <= 1e-12, k


def test_rounding_changes_the_step():
    sd, x, tg, _ = H.case()
    a = T.run(sd, x, tg, H.CASE["C"])
    b = TB.run(sd, x, tg, H.CASE["C"])
    e = sorted(T.rel_l2(b["grads"][k], g) for k, g in a["grads"].items())
    assert e[len(e) // 2] > 1e-5, e


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        return z.clone()

    @staticmethod
    def backward(ctx, dz):
        return TB.rb(dz)


def _straight_through_rb(t):
    return t + (TB.rb(t) - t).detach()


@pytest.mark.parametrize("stride,k", [(1, 3), (2, 3), (1, 1)])
def test_rounded_conv_matches_autograd_through_explicit_rounding(stride, k):
    g = torch.Generator().manual_seed(7 * stride + k)
    x0 = torch.randn(2, 8, 10, 10, generator=g, dtype=torch.float64)
    w0 = torch.randn(6, 8, k, k, generator=g, dtype=torch.float64)
    dz = torch.randn(2, 6, 10 // stride, 10 // stride, generator=g, dtype=torch.float64)
    pad = (k - 1) // 2
    x1, w1 = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    z1 = TB.RoundedConv.apply(x1, w1, stride, pad, True)
    z1.backward(dz)
    x2, w2 = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    z2 = _RoundGrad.apply(F.conv2d(_straight_through_rb(x2), _straight_through_rb(w2), stride=stride, padding=pad))
    z2.backward(dz)
    assert torch.allclose(z1, z2, rtol=1e-13, atol=1e-13)
    assert torch.allclose(x1.grad, x2.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(w1.grad, w2.grad, rtol=1e-12, atol=1e-12)
    # and the rounding is real: dz, x and w all carry more than bf16's 8 bits
    assert not torch.equal(TB.rb(dz), dz) and not torch.equal(TB.rb(x0), x0)


def test_rb_is_torch_bf16_rounding():
    v = torch.tensor([1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -(1.0 + 2 ** -8), 1.0 + 2 ** -8 + 2 ** -20, 2 ** -130, float("inf"), -0.0])
    r = TB.rb(v)
    assert r.tolist()[:5] == [1.0, 1.0 + 2 ** -6, -1.0, 1.0 + 2 ** -7, 2 ** -130]
    assert r[5] == float("inf") and str(r[6].item()) == "-0.0"


def test_backprop_math_defaults_to_f32():
    from yolo_v3_amd import YoloNet, F32, BF16
    from yolo_v3_amd import backprop
    net = YoloNet((96, 96), numClass=3)
    assert net.backprop_math == F32 and net.backprop is False
    assert backprop.backprop_math(net) == F32
    net.backprop_math = BF16
    assert backprop.backprop_math(net) == BF16


@pytest.mark.parametrize("bad", ["F32X3", "F32H2", "garbage", "bf16", True, 1.5, None])
def test_invalid_backprop_math_is_rejected_on_the_host(bad):
    from yolo_v3_amd import YoloNet, F32X3, F32H2, Yv3Error
    from yolo_v3_amd import backprop
    net = YoloNet((96, 96), numClass=3)
    net.backprop_math = {"F32X3": F32X3, "F32H2": F32H2}.get(bad, bad) if isinstance(bad, str) else bad
    with pytest.raises(Yv3Error) as e:
        backprop.backprop_math(net)
    assert e.value.code == _ffi.EINVAL


def _kind(arg):
    arg = arg.strip()
    if "*" in arg:
        return "p"
    base = re.sub(r"\s+\w+$", "", arg)
    return {"int": "i", "long long": "q", "size_t": "z", "float": "f"}[base]


def test_new_prototypes_match_the_header():
    header = open(os.path.join(REPO, "include", "yv3.h")).read()
    ct = {_ffi.c_void_p: "p", _ffi.c_int: "i", _ffi.c_longlong: "q", _ffi.c_size_t: "z", _ffi.c_float: "f"}
    for name in NEW:
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, name
        kinds = [_kind(a) for a in m.group(2).split(",")]
        res, args = _ffi._SIGNATURES[name]
        assert ct[res] == {"int": "i", "size_t": "z"}[m.group(1)], name
        assert [ct[a] for a in args] == kinds, name
