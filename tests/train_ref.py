"""Float64 restatement of one YoloNet training step (reference darknet.py:27-231 in .train() / .eval(), loss.backward()): torch CPU
autograd over F.conv2d, F.batch_norm, LeakyReLU, nearest interpolate and cat, with dL/dlogits from tests/yolo_loss_ref.py.

`run(sd, x, target, ...)` takes a YoloNet state_dict and returns the loss, the three heads' stats, the gradient of every parameter and
the running statistics after the step.  `dtype=torch.float32` gives the same step in fp32 on the CPU, the yardstick behind the GPU
tests' precision bars."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import yolo_loss_ref as R
from yolo_v3_amd import arch


def param_names(sd):
    """Names of the parameters in state_dict order (without the BatchNorm buffers)."""
    return [k for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def leaf_params(sd, dtype, frozen_backbone=False, state=None):
    """The parameters as leaves {name: tensor}: all trainable (but the backbone with frozen_backbone), or as `state.trainable` says."""
    P = {}
    for k in param_names(sd):
        t = sd[k].detach().to(dtype).clone()
        P[k] = t.requires_grad_(state.trainable(k) if state is not None else not (frozen_backbone and k.startswith("feature.")))
    return P


def bn_args(prefix, train, state=None):
    """F.batch_norm's training, momentum and eps for the conv_bn_relu `prefix`: nn.BatchNorm2d's defaults in the mode `train`, or
    what `state.bn(prefix)` says (tests/train_states.py; momentum None is the cumulative average 1 / (num_batches_tracked + 1))."""
    if state is None:
        return dict(training=train, momentum=0.1, eps=1e-5)
    training, momentum, eps, nbt = state.bn(prefix)
    return dict(training=training, momentum=1.0 / (nbt + 1) if momentum is None else momentum, eps=eps)


def forward(sd, x, train=True, dtype=torch.float64, frozen_backbone=False, state=None):
    """-> (logits [3 x [B, 3(5+C), h, w]], leaf parameters {name: tensor}, running statistics after the step {prefix: (mean, var)}).
    With a `state` (tests/train_states.py) it, not train / frozen_backbone, says what is trainable and how each BatchNorm runs."""
    P = leaf_params(sd, dtype, frozen_backbone, state)
    running = {}

    def cbr(prefix, h, stride=1):
        w = P[prefix + ".conv.weight"]
        z = F.conv2d(h, w, stride=stride, padding=(w.shape[-1] - 1) // 2)
        rm, rv = sd[prefix + ".bn.running_mean"].to(dtype).clone(), sd[prefix + ".bn.running_var"].to(dtype).clone()
        y = F.batch_norm(z, rm, rv, P[prefix + ".bn.weight"], P[prefix + ".bn.bias"], **bn_args(prefix, train, state))
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
        return F.conv2d(h, P[name + ".mlist.6.weight"], P[name + ".mlist.6.bias"]), head

    l1, h1 = predet("pre_det1", h)
    u = F.interpolate(cbr("up1.conv", h1), scale_factor=2, mode="nearest")
    l2, h2 = predet("pre_det2", torch.cat((u, r61), 1))
    u = F.interpolate(cbr("up2.conv", h2), scale_factor=2, mode="nearest")
    l3, _ = predet("pre_det3", torch.cat((u, r36), 1))
    return [l1, l2, l3], P, running


def head_losses(logits, target, img_dim_h, num_class):
    """R.yolo_loss of each head on the logits rounded to fp32 (as the network's heads produce them)."""
    return [R.yolo_loss(lg.detach().float().numpy(), np.asarray(target, np.float32), R.ANCHORS, list(arch.ANCHOR_MASKS[k]),
                        img_dim_h, num_class) for k, lg in enumerate(logits)]


def run(sd, x, target, num_class, train=True, dtype=torch.float64, frozen_backbone=False, logits_and_params=None, state=None):
    """One step -> dict(loss, stats (the reference's 9 values summed over the heads, nCorrect/nGT), res (per head), grads, running)."""
    x = torch.as_tensor(x)
    B, img_dim_h = x.shape[0], x.shape[2]
    logits, P, running = logits_and_params or forward(sd, x, train, dtype, frozen_backbone, state)
    res = head_losses(logits, target, img_dim_h, num_class)
    # (every head, unless a state leaves nothing trainable upstream of one)
    heads = [(lg, torch.from_numpy(r["grad"]).to(dtype)) for lg, r in zip(logits, res) if lg.requires_grad]
    torch.autograd.backward([lg for lg, _ in heads], [g for _, g in heads])
    stats = [sum(R.stats_tuple(r, B)[i] for r in res) for i in range(9)]
    return dict(loss=float(sum(float(r["sums"].sum()) for r in res)), stats=stats, res=res,
                grads={k: (p.grad.detach() if p.grad is not None else None) for k, p in P.items()},
                running={k: (m.detach(), v.detach()) for k, (m, v) in running.items()})


def rel_l2(a, ref):
    a, ref = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    n = float(ref.norm())
    return float((a - ref).norm()) / (n if n > 0 else 1.0)
