"""The YOLO loss on the GPU (csrc/yololoss.hip via YoloLayer.forward(x, img_dim, target) and YoloNet.forward(x, target)) against the
reference-produced fixture and the float64 restatement (tests/yolo_loss_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import yolo_loss_ref as R
from tests.helpers import load_sw1_net, trained_like_stream
from tests.test_yolo_loss_host import GOLD, assert_components, assert_grad
from yolo_v3_amd import YoloLayer, _ffi, detect

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_layer(x, spec_mask, img_dim, C, target, grad=False):
    layer = YoloLayer(R.ANCHORS, spec_mask, img_dim, C)
    xt = torch.as_tensor(x).to(DEV)
    if grad:
        xt.requires_grad_(True)
    out = layer(xt, img_dim, torch.as_tensor(target))
    assert len(out) == 10 and out[0].dim() == 0 and out[0].dtype == torch.float32 and out[0].is_cuda
    return xt, out


@pytest.mark.parametrize("spec", R.CASES, ids=[c["name"] for c in R.CASES])
def test_layer_matches_the_reference_fixture(spec):
    gold = np.load(GOLD)
    n, B = spec["name"], spec["B"]
    x, tg = R.make_case(spec, int(gold[n + "/attempt"]))
    xt, out = run_layer(x, spec["mask"], spec["img_dim"], spec["C"], tg, grad=True)
    out[0].backward()
    vals = gold[n + "/values"]
    assert [out[8], out[9]] == list(gold[n + "/counts"])
    assert_components([v * B for v in out[2:8]], vals[2:8] * B)
    assert_components(float(out[0].detach()), vals[0])
    assert_components(out[1], vals[1])
    assert_grad(xt.grad.cpu().numpy(), gold[n + "/grad"])
    res = R.yolo_loss(x, tg, R.ANCHORS, spec["mask"], spec["img_dim"][1], spec["C"])
    assert_grad(xt.grad.cpu().numpy(), res["grad"])


def random_set(seed, B, H, T=50, C=80):
    x = R.synth.uniform(seed, 3, B * 3 * (5 + C) * H * H, -4.0, 4.0).reshape(B, 3, 5 + C, H, H)
    x[:, :, 2:4] *= np.float32(0.4)
    return np.ascontiguousarray(x.reshape(B, 3 * (5 + C), H, H)), R.random_rows(seed, B, T, C, (0.01, 0.9), n_valid_lo=10)


@pytest.mark.parametrize("head", [0, 1, 2])
def test_layer_matches_the_restatement_at_416(head):
    H, mask = (13, 26, 52)[head], ([6, 7, 8], [3, 4, 5], [0, 1, 2])[head]
    x, tg = random_set(100 + head, 8, H)
    xt, out = run_layer(x, mask, (416, 416), 80, tg, grad=True)
    out[0].backward()
    res = R.yolo_loss(x, tg, R.ANCHORS, mask, 416, 80)
    assert res["nGT"] > 8 and out[9] == res["nGT"]
    assert abs(out[8] - res["nCorrect"]) <= res["amb_correct"]
    got = np.array([v * 8 for v in out[2:8]])
    want = res["sums"]
    assert_components(got[[0, 1, 2, 3, 5]], want[[0, 1, 2, 3, 5]])
    assert abs(got[4] - want[4]) <= 1e-5 * abs(want[4]) + res["conf_slack"]
    g = xt.grad.cpu().numpy().astype(np.float64)
    keep = ~res["amb_grad"]
    assert_grad(g[keep], res["grad"][keep])


def test_backward_is_the_kernel_gradient_and_layouts_targets_runs_agree():
    spec = R.CASES[0]
    x, tg = R.make_case(spec, 0)
    layer = YoloLayer(R.ANCHORS, spec["mask"], spec["img_dim"], spec["C"])
    xd = torch.from_numpy(x).to(DEV)
    loss_k, rest_k, grad_k = layer._run_loss(xd, spec["img_dim"], torch.from_numpy(tg), True)
    xt = xd.clone().requires_grad_(True)
    out = layer(xt, spec["img_dim"], torch.from_numpy(tg))
    out[0].backward()
    assert torch.equal(xt.grad, grad_k) and torch.equal(out[0].detach(), loss_k) and tuple(out[1:]) == rest_k
    # CPU and GPU targets, NCHW and channels_last logits, and a second run: the same bits
    out_gpu = layer(xd, spec["img_dim"], torch.from_numpy(tg).to(DEV))
    xl = xd.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out_nhwc = layer(xl, spec["img_dim"], torch.from_numpy(tg))
    out_nhwc[0].backward()
    for o in (out_gpu, out_nhwc):
        assert torch.equal(o[0], loss_k) and tuple(o[1:]) == rest_k
    assert torch.equal(xl.grad, grad_k)
    _, rest2, grad2 = layer._run_loss(xd, spec["img_dim"], torch.from_numpy(tg), True)
    assert rest2 == rest_k and torch.equal(grad2, grad_k)
    # no gradient is computed without requires_grad / under no_grad
    with torch.no_grad():
        o = layer(xt, spec["img_dim"], torch.from_numpy(tg))
    assert not o[0].requires_grad


def test_error_table():
    spec = R.CASES[0]
    x, tg = R.make_case(spec, 0)
    layer = YoloLayer(R.ANCHORS, spec["mask"], spec["img_dim"], spec["C"])
    xd = torch.from_numpy(x).to(DEV)

    def code(t):
        with pytest.raises(_ffi.Yv3Error) as e:
            layer(xd, spec["img_dim"], torch.as_tensor(t))
        return e.value.code

    bad = tg.copy(); bad[0, 0, 0] = 80                  # class >= C
    assert code(bad) == _ffi.EINVAL
    bad = tg.copy(); bad[1, 0, 1] = 1.0                 # cx >= 1
    assert code(bad) == _ffi.EINVAL
    bad = tg.copy(); bad[0, 1, 3] = -0.1                # negative w
    assert code(bad) == _ffi.EINVAL
    assert code(tg[:1]) == _ffi.ESHAPE                  # target batch != x batch
    many = np.zeros((2, _ffi.YOLO_LOSS_MAX_ROWS + 1, 5), np.float32)
    many[:, :, 1:] = 0.25
    assert code(many) == _ffi.ELIMIT
    many[:, -1] = 0                                      # exactly at the limit: accepted
    layer(xd, spec["img_dim"], torch.as_tensor(many))


@pytest.fixture(scope="module")
def trained_net():
    net = load_sw1_net(trained_like_stream()).cuda()
    net.math_mode = _ffi.F32
    return net


def net_inputs():
    x = torch.from_numpy(R.synth.images(4, 416, 4242)).to(DEV)
    tg = R.random_rows(4243, 4, 50, 80, (0.01, 0.9), n_valid_lo=10)
    return x, tg


def test_net_loss_matches_the_restatement_on_head_logits(trained_net):
    net = trained_net
    x, tg = net_inputs()
    before = net(x)
    loss = net(x, torch.from_numpy(tg))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and not loss.requires_grad
    assert list(net.stats) == net.stat_keys
    heads = net.head_logits(x)
    assert [tuple(h.shape) for h in heads] == [(4, 255, 13, 13), (4, 255, 26, 26), (4, 255, 52, 52)]
    tot, n_correct, n_gt, comps, slack = 0.0, 0, 0, np.zeros(6), 0.0
    for h, layer in zip(heads, (net.yolo1, net.yolo2, net.yolo3)):
        res = R.yolo_loss(h.contiguous().cpu().numpy(), tg, layer.anchors_all, layer.anchors_mask, 416, 80)
        comps += res["sums"] / 4
        n_correct += res["nCorrect"]
        n_gt += res["nGT"]
        slack += res["conf_slack"] / 4
    s = net.stats
    assert s["nGT"] == n_gt and n_gt > 0
    got = np.array([s[k] for k in ("loss_x", "loss_y", "loss_w", "loss_h", "loss_conf", "loss_cls")])
    assert_components(got[[0, 1, 2, 3, 5]], comps[[0, 1, 2, 3, 5]])
    assert abs(got[4] - comps[4]) <= 1e-5 * comps[4] + slack
    assert abs(float(loss) / 4 - comps.sum()) <= 1e-5 * comps.sum() + slack
    assert s["recall"] == s["nCorrect"] / s["nGT"]
    # exact F32: the logits plan is the inference plan, and decoding head_logits gives net(x) bit for bit
    dets = torch.cat(before, 1)
    dec = torch.cat([YoloLayer(layer.anchors_all, layer.anchors_mask, (416, 416), 80)(h, (416, 416))
                     for h, layer in zip(heads, (net.yolo1, net.yolo2, net.yolo3))], 1)
    lib = _ffi.lib()
    direct = torch.empty_like(dets)
    row0 = 0
    for h, layer in zip(heads, (net.yolo1, net.yolo2, net.yolo3)):
        nhwc = h.permute(0, 2, 3, 1).contiguous()
        flat = [float(v) for m in layer.anchors_mask for v in layer.anchors_all[m]]
        _ffi.check(lib.yv3_decode(nhwc.data_ptr(), 255, (ctypes.c_float * 6)(*flat), 416.0 / h.shape[2],
                                  direct.data_ptr() + row0 * 85 * 4, direct.shape[1] * 85, 4, h.shape[2], h.shape[3], 80,
                                  _ffi.stream_ptr()), "yv3_decode")
        row0 += h.shape[2] * h.shape[3] * 3
    assert torch.equal(direct, dets)
    assert torch.allclose(dec, dets, rtol=1e-5, atol=1e-5)


def test_math_modes_and_inference_unchanged(trained_net):
    net = trained_net
    x, tg = net_inputs()
    net.math_mode = _ffi.F32
    net(x, torch.from_numpy(tg))
    ref = dict(net.stats)
    for mode in (_ffi.F32H2, _ffi.F32X3, _ffi.BF16):
        net.math_mode = mode
        try:
            dets0 = net.forward_cat(x).clone()
            boxes0 = [b.clone() for b in detect(net, x)]
            loss = net(x, torch.from_numpy(tg))
            s = dict(net.stats)
            dets1 = net.forward_cat(x)
            boxes1 = detect(net, x)
            assert torch.equal(dets0, dets1)
            assert len(boxes0) == len(boxes1) and all(torch.equal(a, b) for a, b in zip(boxes0, boxes1))
        finally:
            net.math_mode = _ffi.F32
        assert s["nGT"] == ref["nGT"]
        assert np.isfinite(float(loss))
        if mode != _ffi.BF16:
            for k in ("loss", "loss_x", "loss_y", "loss_w", "loss_h", "loss_conf", "loss_cls"):
                assert abs(s[k] - ref[k]) <= 1e-4 * abs(ref[k]) + 1e-30, (mode, k, s[k], ref[k])
