"""Float64 reference of every launch of an inference plan, for tests/test_gpu_plan_local.py (and tests/test_plan_ref_host.py, which
pins this file against the oracle on the CPU).

  * ``network_graph``: the 75 convolutions with their producers BY NAME, written down from the reference's wiring (darknet.py:72-88
    backbone with x + conv2(conv1(x)); :107-120 detection branches; :153-162 / :179-194 upsample + concat of the up-conv's output with
    the route) -- independently of engine.Plan, whose descriptor pointers the GPU test compares with it.
  * ``fold_params``: each layer's weight and its BatchNorm (eval) folded in FLOAT64 from the module's own parameters,
    alpha = gamma / sqrt(var + eps), beta = bn_bias - mean * alpha; head convs alpha None, beta = bias, linear.
  * ``launch_ref``: tests/conv_ref.conv_desc_ref of one node on given NHWC inputs -- all rows or a sample.
  * ``fused_pair_ref``: two consecutive nodes whose intermediate is never materialised (the fused front kernels): the first in full,
    the second on the sampled rows, image chunk by image chunk so that the float64 intermediate stays small.
  * ``chain``: the whole network in float64, every layer fed the chain's own outputs.
  * ``torch_f32_rows``: the same launch the way the reference computes it -- torch fp32 on the CPU (F.conv2d + eval BatchNorm +
    LeakyReLU + add) -- the yardstick a launch class's bar is expressed in where the fixed bar does not fit real activations.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from yolo_v3_amd import arch
from tests import conv_ref as cr

BAR = 2e-5            # the project's exact-fp32 bar (tests/test_gpu_conv_matrix.py): |got - ref| <= BAR * max(1, |ref|)
IMAGE = "image"       # the producer name of the first layer's input

Node = namedtuple("Node", "name spec x x2 residual cin_up")
Params = namedtuple("Params", "w alpha beta act bn")          # w fp32 OIHW; alpha / beta float64; bn = (gamma, bias, mean, var, eps) fp32 or None


def network_graph(num_class=80):
    """[Node] in darknet stream order; x / x2 / residual are producer names (x of the first node is IMAGE).  With cin_up > 0 the
    node reads cat(nearest_up2x(x), x2)."""
    specs = arch.conv_specs(num_class)
    nodes = []

    def add(x, x2=None, residual=None, cin_up=0):
        sp = specs[len(nodes)]
        nodes.append(Node(sp.name, sp, x, x2, residual, cin_up))
        return sp.name

    cur = add(IMAGE)
    routes = []
    for nblk in arch.BACKBONE_BLOCKS:
        cur = add(cur)                                          # stride-2 3x3
        for _ in range(nblk):
            mid = add(cur)
            cur = add(mid, residual=cur)                        # x + conv2(conv1(x))
        routes.append(cur)
    r36, r61 = routes[2], routes[3]

    def branch(x, x2=None, cin_up=0):
        route = None
        for j in range(6):
            x = add(x, x2, cin_up=cin_up) if (j == 0 and x2 is not None) else add(x)
            if j == 4:
                route = x
        add(x)                                                  # the plain head conv
        return route

    h1 = branch(cur)
    u1 = add(h1)
    h2 = branch(u1, r61, nodes[-1].spec.cout)
    u2 = add(h2)
    branch(u2, r36, nodes[-1].spec.cout)
    assert len(nodes) == len(specs) == 75
    return nodes


def fold_params(net, num_class=80):
    """{name: Params} from the modules of `net` (any device), BatchNorm folded in float64."""
    out = {}
    for sp in arch.conv_specs(num_class):
        m = net.get_submodule(sp.name)
        if isinstance(m, torch.nn.Conv2d):
            assert not sp.bn
            out[sp.name] = Params(m.weight.detach().float().cpu(), None, m.bias.detach().double().cpu(), cr.ACT_LINEAR, None)
            continue
        bn = m.bn
        g, b = bn.weight.detach().cpu(), bn.bias.detach().cpu()
        mean, var = bn.running_mean.detach().cpu(), bn.running_var.detach().cpu()
        alpha = g.double() / torch.sqrt(var.double() + float(bn.eps))
        beta = b.double() - mean.double() * alpha
        out[sp.name] = Params(m.conv.weight.detach().float().cpu(), alpha, beta, cr.ACT_LEAKY,
                              (g.float(), b.float(), mean.float(), var.float(), float(bn.eps)))
    return out


def launch_ref(node, p, x, x2=None, residual=None, pixels=None):
    """float64 [M or len(pixels), cout] of one node on NHWC inputs (x the low-resolution map when node.cin_up)."""
    return cr.conv_desc_ref(x, p.w, p.beta, p.alpha, residual, x2, node.cin_up, node.spec.stride, p.act, pixels)


def out_shape(node, B, H, W):
    ho, wo = cr.out_hw(H, W, node.spec.k, node.spec.stride)
    return B, ho, wo, node.spec.cout


def rows_of(B, Ho, Wo, seed, full_below=8192):
    """conv_ref.sample_rows, or every row where the launch is small."""
    M = B * Ho * Wo
    return torch.arange(M) if M <= full_below else cr.sample_rows(B, Ho, Wo, seed=seed)


def fused_pair_ref(first, pf, second, ps, x, rows, residual=None, chunk=4):
    """`second(first(x))` on the output rows `rows` of `second` (float64 [len(rows), cout]); `first` is computed in full, `chunk` images at
    a time.  x NHWC [B, H, W, cin]; residual (of `second`) NHWC or None."""
    assert not first.cin_up and not second.cin_up and first.residual is None
    B, H, W = x.shape[0], x.shape[1], x.shape[2]
    _, h1, w1, c1 = out_shape(first, B, H, W)
    _, h2, w2, c2 = out_shape(second, B, h1, w1)
    rows = torch.as_tensor(rows, dtype=torch.long)
    out = torch.empty(rows.numel(), c2, dtype=torch.float64)
    img = rows // (h2 * w2)
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        sel = ((img >= b0) & (img < b1)).nonzero().reshape(-1)
        if not sel.numel():
            continue
        mid = launch_ref(first, pf, x[b0:b1]).reshape(b1 - b0, h1, w1, c1)
        res = residual[b0:b1] if residual is not None else None
        out[sel] = launch_ref(second, ps, mid, residual=res, pixels=rows[sel] - b0 * h2 * w2)
    return out


def chain(params, image_nchw, graph=None):
    """{name: float64 NHWC output} of the whole network, every node fed the chain's own float64 outputs."""
    graph = graph or network_graph()
    acts = {IMAGE: image_nchw.double().permute(0, 2, 3, 1).contiguous()}
    for n in graph:
        x = acts[n.x]
        B, H, W = (x.shape[0], x.shape[1] * 2, x.shape[2] * 2) if n.cin_up else tuple(x.shape[:3])
        y = launch_ref(n, params[n.name], x, acts.get(n.x2), acts.get(n.residual))
        acts[n.name] = y.reshape(out_shape(n, B, H, W))
    del acts[IMAGE]
    return acts


def torch_f32_rows(node, p, x, x2=None, residual=None, pixels=None):
    """The node as the reference's modules compute it on the CPU: fp32 F.conv2d, eval F.batch_norm, LeakyReLU(0.1), + residual
    (darknet.py:34-53, :161-162), on fp32 NHWC inputs -> fp32 [M or len(pixels), cout]."""
    xin = x.float().permute(0, 3, 1, 2)
    if node.cin_up:
        xin = torch.cat((F.interpolate(xin, scale_factor=2, mode="nearest"), x2.float().permute(0, 3, 1, 2)), 1)
    pad = (node.spec.k - 1) // 2
    if p.bn is None:
        y = F.conv2d(xin, p.w, p.beta.float(), node.spec.stride, pad)
    else:
        g, b, mean, var, eps = p.bn
        y = F.leaky_relu(F.batch_norm(F.conv2d(xin, p.w, None, node.spec.stride, pad), mean, var, g, b, False, 0.0, eps), 0.1)
    if residual is not None:
        y = y + residual.float().permute(0, 3, 1, 2)
    y = y.permute(0, 2, 3, 1).reshape(-1, node.spec.cout)
    return y if pixels is None else y[torch.as_tensor(pixels, dtype=torch.long)]


def norm_err(got, ref):
    """|got - ref| / max(1, |ref|), float64."""
    ref = ref.double()
    return (got.double() - ref).abs() / ref.abs().clamp(min=1.0)
