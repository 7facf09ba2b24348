"""Float64 restatement of one BF16 training step (net.backprop_math = BF16; yolo_v3_amd/backprop.py, csrc/train_bf16.hip).

The step is tests/train_ref.py's with one change: every convolution rounds its two operands to bf16 (round to nearest even, as
``torch.Tensor.to(torch.bfloat16)`` rounds an fp32 value) -- forward conv(rb(x), rb(w)); backward dx from rb(dz) and rb(w), dw from
rb(x) and rb(dz) -- and computes the products in `dtype`.  Everything else (BatchNorm, LeakyReLU, sums, the upsample and the loss)
is train_ref's.  `forward` restates train_ref.forward with a pluggable convolution; `run` reuses train_ref.run's loss and backward.
`dtype=torch.float32` gives the same rounded step in fp32 on the CPU, the yardstick behind the GPU tests' precision bars."""
import torch
import torch.nn.functional as F

from tests import train_ref as T
from yolo_v3_amd import arch

param_names, head_losses, rel_l2 = T.param_names, T.head_losses, T.rel_l2


def rb(t):
    """t rounded to bf16 through its fp32 value (the GPU rounds the fp32 tensors it holds), in t's dtype."""
    return t.float().to(torch.bfloat16).to(t.dtype)


class RoundedConv(torch.autograd.Function):
    """conv2d whose forward and backward products take bf16-rounded operands (rounding = False: plain conv2d)."""

    @staticmethod
    def forward(ctx, x, w, stride, padding, rounding):
        xr, wr = (rb(x), rb(w)) if rounding else (x, w)
        ctx.save_for_backward(xr, wr)
        ctx.stride, ctx.padding, ctx.rounding = stride, padding, rounding
        return F.conv2d(xr, wr, stride=stride, padding=padding)

    @staticmethod
    def backward(ctx, dz):
        xr, wr = ctx.saved_tensors
        dzr = rb(dz) if ctx.rounding else dz
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.nn.grad.conv2d_input(xr.shape, wr, dzr, stride=ctx.stride, padding=ctx.padding)
        if ctx.needs_input_grad[1]:
            dw = torch.nn.grad.conv2d_weight(xr, wr.shape, dzr, stride=ctx.stride, padding=ctx.padding)
        return dx, dw, None, None, None


def rounded_conv(rounding=True):
    def conv(h, w, bias=None, stride=1):
        z = RoundedConv.apply(h, w, stride, (w.shape[-1] - 1) // 2, rounding)
        return z if bias is None else z + bias.view(1, -1, 1, 1)
    return conv


def forward(sd, x, train=True, dtype=torch.float64, frozen_backbone=False, conv=None, state=None):
    """train_ref.forward with `conv(h, w, bias, stride)` in place of F.conv2d (default: the bf16-rounding conv)."""
    conv = conv or rounded_conv(True)
    P = T.leaf_params(sd, dtype, frozen_backbone, state)
    running = {}

    def cbr(prefix, h, stride=1):
        z = conv(h, P[prefix + ".conv.weight"], None, stride)
        rm, rv = sd[prefix + ".bn.running_mean"].to(dtype).clone(), sd[prefix + ".bn.running_var"].to(dtype).clone()
        y = F.batch_norm(z, rm, rv, P[prefix + ".bn.weight"], P[prefix + ".bn.bias"], **T.bn_args(prefix, train, state))
        running[prefix] = (rm, rv)
        return F.leaky_relu(y, 0.1)

    h = cbr("feature.mlist.0", torch.as_tensor(x).to(dtype))
    pos, routes = 1, []
    for nb in arch.BACKBONE_BLOCKS:
        h = cbr("feature.mlist.%d" % pos, h, 2)
        pos += 1
        for _ in range(nb):
            h = h + cbr("feature.mlist.%d.conv2" % pos, cbr("feature.mlist.%d.conv1" % pos, h))
            pos += 1
        routes.append(h)
    r36, r61 = routes[2], routes[3]

    def predet(name, h):
        for i in range(6):
            h = cbr("%s.mlist.%d" % (name, i), h)
            if i == 4:
                head = h
        return conv(h, P[name + ".mlist.6.weight"], P[name + ".mlist.6.bias"], 1), head

    l1, h1 = predet("pre_det1", h)
    u = F.interpolate(cbr("up1.conv", h1), scale_factor=2, mode="nearest")
    l2, h2 = predet("pre_det2", torch.cat((u, r61), 1))
    u = F.interpolate(cbr("up2.conv", h2), scale_factor=2, mode="nearest")
    l3, _ = predet("pre_det3", torch.cat((u, r36), 1))
    return [l1, l2, l3], P, running


def run(sd, x, target, num_class, train=True, dtype=torch.float64, frozen_backbone=False, rounding=True, state=None):
    """One BF16 step (rounding = False: the F32 step) -> train_ref.run's dict."""
    x = torch.as_tensor(x)
    fw = forward(sd, x, train, dtype, frozen_backbone, conv=rounded_conv(rounding), state=state)
    return T.run(sd, x, target, num_class, train=train, dtype=dtype, frozen_backbone=frozen_backbone, logits_and_params=fw)
