"""Float64 restatement of one BF16_ACT training step (net.backprop_math = BF16_ACT; yolo_v3_amd/backprop.py, csrc/train_bf16.hip,
csrc/train_bf16_act.hip).

The step is tests/train_ref_bf16.py's (every convolution product takes bf16-rounded operands, the backward's dz included) with the
activations stored in bf16 only, i.e. with two more roundings per conv_bn_relu layer:

* the conv output: ``zb = rb(conv(rb(x), rb(w)))``; the batch statistics, the running statistics and the BatchNorm read zb;
* the layer output: ``rb(leaky(bn(zb)))``, or ``rb(leaky(bn(zb)) + res)`` in a residual block, `res` being the stored (rounded)
  output of the earlier layer.

The head logits are not rounded.  The gradient of a rounding is the identity (straight-through): the backward is train_ref_bf16's,
evaluated at the rounded activations.  ``act_rounding=False`` switches the two roundings off and leaves train_ref_bf16's step;
``dtype=torch.float32`` gives the same step in fp32 on the CPU, the yardstick behind the GPU tests' bars."""
import torch
import torch.nn.functional as F

from tests import train_ref as T
from tests import train_ref_bf16 as TB
from yolo_v3_amd import arch

param_names, head_losses, rel_l2, rb = T.param_names, T.head_losses, T.rel_l2, TB.rb


class _RoundST(torch.autograd.Function):
    """rb(t) with the identity as its gradient."""

    @staticmethod
    def forward(ctx, t):
        return rb(t)

    @staticmethod
    def backward(ctx, g):
        return g


def forward(sd, x, train=True, dtype=torch.float64, frozen_backbone=False, act_rounding=True, x_requires_grad=False, state=None):
    """train_ref_bf16.forward with the stored activations rounded -> (logits, leaf parameters, running statistics after the step);
    with x_requires_grad the input is a leaf too, returned under the key "x" of the parameters."""
    conv = TB.rounded_conv(True)
    st = _RoundST.apply if act_rounding else (lambda t: t)
    P = T.leaf_params(sd, dtype, frozen_backbone, state)
    running = {}

    def cbr(prefix, h, stride=1, res=None):
        zb = st(conv(h, P[prefix + ".conv.weight"], None, stride))
        rm, rv = sd[prefix + ".bn.running_mean"].to(dtype).clone(), sd[prefix + ".bn.running_var"].to(dtype).clone()
        y = F.batch_norm(zb, rm, rv, P[prefix + ".bn.weight"], P[prefix + ".bn.bias"], **T.bn_args(prefix, train, state))
        running[prefix] = (rm, rv)
        y = F.leaky_relu(y, 0.1)
        return st(y if res is None else y + res)

    x0 = torch.as_tensor(x).to(dtype)
    if x_requires_grad:
        x0 = x0.clone().requires_grad_(True)
    h = cbr("feature.mlist.0", x0)
    pos, routes = 1, []
    for nb in arch.BACKBONE_BLOCKS:
        h = cbr("feature.mlist.%d" % pos, h, 2)
        pos += 1
        for _ in range(nb):
            h = cbr("feature.mlist.%d.conv2" % pos, cbr("feature.mlist.%d.conv1" % pos, h), res=h)
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
    if x_requires_grad:
        P["x"] = x0
    return [l1, l2, l3], P, running


def run(sd, x, target, num_class, train=True, dtype=torch.float64, frozen_backbone=False, act_rounding=True, x_requires_grad=False,
        state=None):
    """One BF16_ACT step (act_rounding = False: the BF16 step) -> train_ref.run's dict; grads["x"] with x_requires_grad."""
    x = torch.as_tensor(x)
    fw = forward(sd, x, train, dtype, frozen_backbone, act_rounding, x_requires_grad, state)
    return T.run(sd, x, target, num_class, train=train, dtype=dtype, frozen_backbone=frozen_backbone, logits_and_params=fw)
