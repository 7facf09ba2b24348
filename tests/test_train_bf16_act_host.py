"""The BF16_ACT training step's host side (CPU only): the float64 restatement tests/train_ref_bf16_act.py against
tests/train_ref_bf16.py, net.backprop_math's new value, and the new C-ABI (exported by the built library, prototypes as the header)."""
import ctypes
import os
import re

import pytest
import torch

from tests import test_train_host as H
from tests import train_ref_bf16 as TB
from tests import train_ref_bf16_act as TA
from tests import yolo_loss_ref as R
from tests.test_train_bf16_host import _kind
from yolo_v3_amd import _ffi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("yv3_train_conv_fwd_bf16o", "yv3_train_channel_bf16_workspace_bytes", "yv3_train_bn_stats_bf16", "yv3_train_bn_act_fwd_bf16",
       "yv3_train_bn_act_bwd_bf16", "yv3_train_bias_bwd_bf16")


C = H.CASE["C"]


@pytest.fixture(scope="module")
def case64():
    """(state_dict, x, target) at 64x64, bs=2, and the BF16 step on it."""
    from yolo_v3_amd import synth
    sd = H.state_dict()
    x = synth.images(2, 64, 31)
    tg = R.random_rows(53, 2, 8, C, (0.05, 0.7))
    return sd, x, tg, TB.run(sd, x, tg, C)


def test_restatement_without_the_activation_roundings_is_the_bf16_step(case64):
    sd, x, tg, a = case64
    assert tuple(x.shape) == (2, 3, 64, 64)
    b = TA.run(sd, x, tg, C, act_rounding=False)
    assert abs(a["loss"] - b["loss"]) <= 1e-13 * abs(a["loss"])
    assert a["stats"] == b["stats"]
    for k, g in a["grads"].items():
        assert TA.rel_l2(b["grads"][k], g) <= 1e-13, k
    for k, (m, v) in a["running"].items():
        assert TA.rel_l2(b["running"][k][0], m) <= 1e-13 and TA.rel_l2(b["running"][k][1], v) <= 1e-13, k


def test_the_activation_roundings_change_the_step(case64):
    sd, x, tg, bf16_step = case64
    b = TA.run(sd, x, tg, C)
    e = sorted(TA.rel_l2(b["grads"][k], g) for k, g in bf16_step["grads"].items())
    assert e[len(e) // 2] > 1e-5, e
    assert b["loss"] != bf16_step["loss"]


def test_the_rounding_is_straight_through():
    t = torch.tensor([1.0 + 2 ** -8 + 2 ** -20, -3.3, 2.0 ** -130], dtype=torch.float64, requires_grad=True)
    y = TA._RoundST.apply(t)
    assert torch.equal(y.detach(), TB.rb(t.detach())) and not torch.equal(y.detach(), t.detach())
    g = torch.tensor([0.3, -7.0, 1e-30], dtype=torch.float64)
    y.backward(g)
    assert torch.equal(t.grad, g)


def test_the_input_gradient_is_a_leaf_of_the_restatement(case64):
    sd, x, tg, _ = case64
    r = TA.run(sd, x, tg, C, x_requires_grad=True)
    assert tuple(r["grads"]["x"].shape) == tuple(x.shape) and float(r["grads"]["x"].abs().max()) > 0


def test_backprop_math_accepts_bf16_act():
    from yolo_v3_amd import YoloNet, F32, BF16, F32X3, F32H2, BF16_ACT
    from yolo_v3_amd import backprop
    assert BF16_ACT not in (F32, BF16, F32X3, F32H2) and BF16_ACT == _ffi.BF16_ACT
    net = YoloNet((96, 96), numClass=3)
    net.backprop_math = BF16_ACT
    assert backprop.backprop_math(net) == BF16_ACT


@pytest.mark.parametrize("bad", ["F32X3", "F32H2", "garbage", "bf16_act", True, 4.0, 5, -1, None])
def test_invalid_backprop_math_is_still_rejected_on_the_host(bad):
    from yolo_v3_amd import YoloNet, F32X3, F32H2, Yv3Error
    from yolo_v3_amd import backprop
    net = YoloNet((96, 96), numClass=3)
    net.backprop_math = {"F32X3": F32X3, "F32H2": F32H2}.get(bad, bad) if isinstance(bad, str) else bad
    with pytest.raises(Yv3Error) as e:
        backprop.backprop_math(net)
    assert e.value.code == _ffi.EINVAL


def test_the_built_library_exports_the_new_symbols():
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert hasattr(handle, name) and name in _ffi.EXPORTS, name
    # the host-side argument checks answer before any launch (no GPU is touched: every call below is refused)
    lib = _ffi.lib()
    assert lib.yv3_train_channel_bf16_workspace_bytes(0, 8) == 0 and lib.yv3_train_channel_bf16_workspace_bytes(4, 0) == 0
    assert lib.yv3_train_channel_bf16_workspace_bytes(100, 255) > 0
    p = 4096                                    # (a non-null pointer that is never dereferenced)
    assert lib.yv3_train_conv_fwd_bf16o(p, None, p, p, 1, 8, 8, 8, 0, 12, 3, 1, 0, None) == _ffi.ESHAPE
    assert lib.yv3_train_conv_fwd_bf16o(p, None, p, None, 1, 8, 8, 8, 0, 16, 3, 1, 0, None) == _ffi.EINVAL
    assert lib.yv3_train_bn_stats_bf16(p, 4, 12, 1e-5, 0.1, None, None, None, None, p, p, p, 1 << 20, None) == _ffi.ESHAPE
    assert lib.yv3_train_bn_stats_bf16(p, 4, 16, 1e-5, 0.1, None, None, None, None, p, p, p, 8, None) == _ffi.EWORKSPACE
    assert lib.yv3_train_bn_act_fwd_bf16(p, p, p, p, p, None, p, 4, 12, None) == _ffi.ESHAPE
    assert lib.yv3_train_bn_act_fwd_bf16(p, p, p, p, p, None, None, 4, 16, None) == _ffi.EINVAL
    assert lib.yv3_train_bn_act_bwd_bf16(p, p, p, p, p, p, p, p, p, 4, 12, 1, p, 1 << 20, None) == _ffi.ESHAPE
    assert lib.yv3_train_bn_act_bwd_bf16(p, p, p, p, p, p, p, p, p, 4, 16, 1, p, 8, None) == _ffi.EWORKSPACE
    assert lib.yv3_train_bias_bwd_bf16(p, None, p, p, 0, 255, p, 1 << 20, None) == _ffi.EINVAL
    assert lib.yv3_train_bias_bwd_bf16(p, None, p, p, 4, 255, p, 8, None) == _ffi.EWORKSPACE


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
