"""The F16 math mode's definition, evaluated on the CPU: oracle_cpu's ``prec="bf16"`` trunk with fp16 in place of bfloat16.

  * weights of every conv except the 3-channel first layer: each output channel scaled to max|w_row| in [1, 2) by an exact power of two
    (engine.pack_conv), rounded to fp16 (nearest even, subnormals kept), the inverse scale applied to the conv's fp32 result;
  * every STORED activation rounded to fp16 once and saturated to +-65504: each conv_bn_relu output, each residual sum after its fp32 add,
    the upsample group's conv output;
  * everything else fp32: accumulation, BatchNorm, LeakyReLU, the residual add, the head logits, decode and post-processing.

Same torch ops in the same order as oracle/oracle_cpu.py.  ``scale=False`` leaves the weight scale out: the weights are rounded as they
are (tiny weights of a row then become fp16 subnormals), and the evaluation is oracle_cpu's ``prec="bf16"`` trunk with fp16 as its
rounding function, op for op -- the measurement the mode was proposed on, which tests/test_f16_host.py reproduces with it."""
import torch
import torch.nn.functional as F

from oracle import oracle_cpu as oc

F16_MAX = 65504.0


def round_f16(t):
    """fp32 -> nearest fp16 (ties to even, subnormals kept), saturated to +-65504 -> fp32."""
    return t.clamp(-F16_MAX, F16_MAX).half().float()


def round_weight(w):
    """(fp16-rounded scaled weights, per-output-channel inverse scale): w ~ wq * inv.view(-1, 1, 1, 1), both factors exact in fp32."""
    wmax = w.abs().amax(dim=(1, 2, 3))
    e = torch.where(wmax > 0, -torch.floor(torch.log2(wmax.clamp(min=1e-38))), torch.zeros_like(wmax)).clamp(-100.0, 100.0)
    return round_f16(w * torch.exp2(e).view(-1, 1, 1, 1)), torch.exp2(-e)


def _conv(x, w, stride=1, scale=True, bias=None):
    pad = (w.shape[2] - 1) // 2
    if w.shape[1] == 3:
        return F.conv2d(x, w, bias, stride, pad)
    if not scale:
        return F.conv2d(x, round_f16(w), bias, stride, pad)
    wq, inv = round_weight(w)
    y = F.conv2d(x, wq, None, stride, pad) * inv.view(1, -1, 1, 1)
    return y if bias is None else y + bias.view(1, -1, 1, 1)


def cbr(sd, prefix, x, stride=1, store=True, stats=None, scale=True):
    y = _conv(x, sd[prefix + ".conv.weight"], stride, scale)
    y = F.batch_norm(y, sd[prefix + ".bn.running_mean"], sd[prefix + ".bn.running_var"],
                     sd[prefix + ".bn.weight"], sd[prefix + ".bn.bias"], False, 0.1, 1e-5)
    y = F.leaky_relu(y, 0.1)
    if not store:
        return y
    if stats is not None:
        stats["max_stored"] = max(stats.get("max_stored", 0.0), float(y.abs().max()))
    return round_f16(y)


def head_logits(sd, x, stats=None, scale=True):
    """The three head logit maps [B, 3*(5+C), h, w] in fp32.  stats (a dict): receives max_stored, the largest stored |activation|."""
    def layer(prefix, t, stride=1, store=True):
        return cbr(sd, prefix, t, stride, store, stats, scale)

    def store(t):
        if stats is not None:
            stats["max_stored"] = max(stats.get("max_stored", 0.0), float(t.abs().max()))
        return round_f16(t)

    x = layer("feature.mlist.0", x)
    idx, routes = 1, {}
    for nblk in oc.BLOCKS:
        x = layer("feature.mlist.%d" % idx, x, stride=2)
        idx += 1
        for _ in range(nblk):
            p = "feature.mlist.%d" % idx
            h = layer(p + ".conv1", x)
            x = store(x + layer(p + ".conv2", h, store=False))
            idx += 1
        routes[idx - 1] = x
    r36, r61 = routes[14], routes[23]

    def predet(prefix, t):
        route = None
        for i in range(6):
            t = layer("%s.mlist.%d" % (prefix, i), t)
            if i == 4:
                route = t
        return _conv(t, sd[prefix + ".mlist.6.weight"], 1, scale, sd[prefix + ".mlist.6.bias"]), route

    def upcat(prefix, head, tail):
        return torch.cat((F.interpolate(layer(prefix + ".conv", head), scale_factor=2, mode="nearest"), tail), 1)

    l1, h1 = predet("pre_det1", x)
    l2, h2 = predet("pre_det2", upcat("up1", h1, r61))
    l3, _ = predet("pre_det3", upcat("up2", h2, r36))
    return l1, l2, l3


def yolonet_forward(sd, x, anchors=oc.DEFAULT_ANCHORS, num_class=80):
    """(det1, det2, det3) of the F16 definition: the fp32 decode of oracle_cpu on head_logits."""
    img_dim = (x.shape[3], x.shape[2])
    l1, l2, l3 = head_logits(sd, x)
    return (oc.decode(l1, anchors, (6, 7, 8), img_dim, num_class), oc.decode(l2, anchors, (3, 4, 5), img_dim, num_class),
            oc.decode(l3, anchors, (0, 1, 2), img_dim, num_class))


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())
