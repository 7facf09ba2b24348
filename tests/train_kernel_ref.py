"""Float64 restatements of the training kernels' operations, one op at a time (csrc/train.hip, csrc/train_bf16.hip), with the error
model each is held to, and the same per-op references chained over YoloNet's graph (yolo_v3_amd/backprop.py).  CPU torch only.

Used by tests/test_gpu_train_edges.py (each C-ABI entry point at the edges of its tiling), tests/test_gpu_train_local.py (every op of
a real step on the inputs the GPU fed it) and tests/test_train_kernel_ref_host.py (the chain reproduces tests/train_ref.py's autograd
step, which pins these restatements to the reference's step).

Bars.  CONV_BAR bounds a conv product per element: |got - ref| <= CONV_BAR * sum|a||b|, the sum taken by the same float64 op on the
absolute values (an fp32 MFMA chain; for BF16 the operands are the bf16-rounded values, whose products are exact in fp32).  BN_BAR
bounds elementwise / per-channel fp32 results on well-conditioned data: |got - ref| <= BN_BAR * max|ref|.

The LeakyReLU kink.  dz, dgamma and dbeta are discontinuous where u = gamma*xhat + beta crosses 0, and the kernel decides the side in
fp32.  An element is *undecided* when |u| <= KINK * (|gamma*xhat| + |beta|) in float64: its dz is not compared, and since the other
side changes du by 0.9*|dy|, its channel's dbeta may move by 0.9*|dy| and dgamma by 0.9*|dy|*|xhat|: both tolerances grow by
S_c = sum over the channel's undecided elements of 0.9*|dy|*max(1, |xhat|).  In train mode dz_i = coef*(du_i - dbeta/P - xhat_i*
dgamma/P) moves by at most |coef|/P * (1 + |xhat_i|) * S_c; its tolerance grows by that, and never by more than S_c.  The share of
undecided elements must stay <= KINK_SHARE (asserted by the callers): the rule is a condition, not a loophole."""
import torch
import torch.nn.functional as F

CONV_BAR = 2e-6
BN_BAR = 1e-5
KINK = 4e-6
KINK_SHARE = 1e-4
EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.1


def rb(t):
    """t rounded to bf16 through its fp32 value, in t's dtype (tests/train_ref_bf16.py's rounding)."""
    return t.float().to(torch.bfloat16).to(t.dtype)


# ---------------------------------------------------------------- convolution products (NCHW float64) -> (value, sum|a||b|)
def conv_fwd(x, w, stride, bias=None):
    p = (w.shape[-1] - 1) // 2
    z = F.conv2d(x, w, bias, stride=stride, padding=p)
    s = F.conv2d(x.abs(), w.abs(), None if bias is None else bias.abs(), stride=stride, padding=p)
    return z, s


def conv_dgrad(xshape, w, dz, stride):
    p = (w.shape[-1] - 1) // 2
    return (torch.nn.grad.conv2d_input(xshape, w, dz, stride=stride, padding=p),
            torch.nn.grad.conv2d_input(xshape, w.abs(), dz.abs(), stride=stride, padding=p))


def conv_wgrad(x, wshape, dz, stride):
    p = (wshape[-1] - 1) // 2
    return (torch.nn.grad.conv2d_weight(x, wshape, dz, stride=stride, padding=p),
            torch.nn.grad.conv2d_weight(x.abs(), wshape, dz.abs(), stride=stride, padding=p))


def upcat(low, tail):
    """cat(up2x(low), tail) along the channels (NCHW)."""
    return torch.cat((F.interpolate(low, scale_factor=2, mode="nearest"), tail), 1)


def upcat_bwd(dcat, cu):
    """-> (dlow, sum of |.| behind dlow, dtail): dlow sums each 2x2 block of the first cu channels."""
    B, _, H, W = dcat.shape
    blk = dcat[:, :cu].reshape(B, cu, H // 2, 2, W // 2, 2)
    return blk.sum((3, 5)), blk.abs().sum((3, 5)), dcat[:, cu:]


def rows(t):
    """NCHW -> [P, C] (the kernels' NHWC rows)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def unrows(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


# ---------------------------------------------------------------- BatchNorm + LeakyReLU on [P, C] float64
def bn_batch_stats(z, eps=EPS):
    """-> (mean, biased variance, 1/sqrt(var + eps)) of each column."""
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def bn_running(mean, var, P, run_mean, run_var, momentum=MOMENTUM):
    """nn.BatchNorm2d's update: the unbiased variance (for P = 1 the kernel keeps the biased one, 0)."""
    unb = var * (P / (P - 1.0)) if P > 1 else var
    return (1 - momentum) * run_mean + momentum * mean, (1 - momentum) * run_var + momentum * unb


def bn_eval_stats(run_mean, run_var, eps=EPS):
    return run_mean, 1.0 / torch.sqrt(run_var + eps)


def bn_act_fwd(z, mean, invstd, gamma, beta, res=None):
    u = gamma * ((z - mean) * invstd) + beta
    y = torch.where(u > 0, u, u * SLOPE)
    return y if res is None else y + res


def bn_act_bwd(z, dy, mean, invstd, gamma, beta, train):
    """-> dict(dz, dgamma, dbeta, und (undecided mask), S (per-channel growth), dz_growth (per element), share)."""
    P = z.shape[0]
    xhat = (z - mean) * invstd
    gx = gamma * xhat
    u = gx + beta
    und = u.abs() <= KINK * (gx.abs() + beta.abs())
    du = torch.where(u > 0, dy, dy * SLOPE)
    dbeta, dgamma = du.sum(0), (du * xhat).sum(0)
    coef = gamma * invstd
    dz = coef * (du - dbeta / P - xhat * (dgamma / P)) if train else coef * du
    S = (und * ((1 - SLOPE) * dy.abs() * xhat.abs().clamp(min=1.0))).sum(0)
    growth = torch.minimum(S.expand_as(z), coef.abs() / P * (1 + xhat.abs()) * S) if train else torch.zeros_like(z)
    return dict(dz=dz, dgamma=dgamma, dbeta=dbeta, und=und, S=S, dz_growth=growth, share=float(und.double().mean()))


def bias_bwd(dlogits, scale=None):
    """-> (dout, dbias, column sums of |dout|); dout is one fp32 multiply (compare it against dout.float() exactly)."""
    dout = dlogits if scale is None else dlogits * scale
    dout = dout.float().double()
    return dout, dout.sum(0), dout.abs().sum(0)


# ---------------------------------------------------------------- comparison (-> worst error / tolerance; <= 1 passes)
def ratio(got, ref, tol):
    """max |got - ref| / tol over the elements (tol: tensor or number, > 0 wherever it matters)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), "non-finite"
    d = (got - ref).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(d)
    r = torch.where(d == 0, torch.zeros_like(d), d / tol.clamp(min=1e-300))
    return float(r.max()) if r.numel() else 0.0


def conv_ratio(got, ref, scale):
    return ratio(got, ref, CONV_BAR * scale + 1e-30)


def bn_ratio(got, ref, growth=0.0, mask=None, bar=BN_BAR):
    """BN_BAR * max|ref| (+ growth) per element; `mask`: elements left out (undecided dz)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    tol = bar * max(float(ref.abs().max()), 1e-30) + torch.as_tensor(growth, dtype=torch.float64)
    if mask is not None:
        got = torch.where(mask, ref, got)
    return ratio(got, ref, tol)


def bn_bwd_ratios(got_dz, got_dgamma, got_dbeta, ref, bar=BN_BAR):
    """{name: ratio} of a bn_act_bwd result against bn_act_bwd()'s dict under the kink rule."""
    return dict(dz=bn_ratio(got_dz, ref["dz"], ref["dz_growth"], ref["und"], bar),
                dgamma=bn_ratio(got_dgamma, ref["dgamma"], ref["S"], None, bar),
                dbeta=bn_ratio(got_dbeta, ref["dbeta"], ref["S"], None, bar))


# ---------------------------------------------------------------- the per-op references chained over YoloNet's graph
def op_params(net, ops):
    """Per op of backprop.graph(net): (weight key, bias key or None, bn prefix or None) in state_dict names."""
    names = {id(m): n for n, m in net.named_modules()}
    out = []
    for op in ops:
        n = names[id(op.module)]
        out.append((n + ".weight", n + ".bias", None) if op.head else (n + ".conv.weight", None, n + ".bn"))
    return out


def chain_step(net, sd, x, dlogits_of, train=True, rounding=False):
    """One training step as backprop.forward / backward string it together, every op from the functions above in float64.
    sd: state_dict (any dtype); x: [B, 3, H, W]; dlogits_of(logits) -> the three dL/dlogits (NCHW float64).
    -> dict(logits, grads {state_dict key: tensor}, running {bn prefix: (mean, var)})."""
    from yolo_v3_amd import backprop
    ops = backprop.graph(net)
    keys = op_params(net, ops)
    r = rb if rounding else (lambda t: t)
    P = {k: v.detach().double() for k, v in sd.items()}
    bufs, saved, running = {"x": torch.as_tensor(x).double()}, {}, {}

    def conv_in(op):
        return bufs[op.src] if op.src2 is None else upcat(bufs[op.src2], bufs[op.src])

    for i, (op, (kw, kb, kbn)) in enumerate(zip(ops, keys)):
        st = op.conv.stride[0]
        z, _ = conv_fwd(r(conv_in(op)), r(P[kw]), st, P[kb] if kb else None)
        if op.head:
            bufs[op.out] = z
            continue
        B, _, H, W = z.shape
        zr = rows(z)
        if train:
            mean, var, invstd = bn_batch_stats(zr)
            running[kbn] = bn_running(mean, var, zr.shape[0], P[kbn + ".running_mean"], P[kbn + ".running_var"])
        else:
            mean, invstd = bn_eval_stats(P[kbn + ".running_mean"], P[kbn + ".running_var"])
            running[kbn] = (P[kbn + ".running_mean"], P[kbn + ".running_var"])
        res = rows(bufs[op.res]) if op.res is not None else None
        bufs[op.out] = unrows(bn_act_fwd(zr, mean, invstd, P[kbn + ".weight"], P[kbn + ".bias"], res), B, H, W)
        saved[i] = (zr, mean, invstd)
    heads = sorted((op for op in ops if op.head), key=lambda o: o.head_idx)
    logits = [bufs[op.out] for op in heads]
    grads = {op.out: g.double() for op, g in zip(heads, dlogits_of(logits))}
    pg = {}

    def give(buf, t):
        grads[buf] = grads[buf] + t if buf in grads else t

    for i in range(len(ops) - 1, -1, -1):
        op, (kw, kb, kbn) = ops[i], keys[i]
        dy = grads.pop(op.out)
        B, _, Ho, Wo = dy.shape
        st = op.conv.stride[0]
        if op.head:
            dz = dy
            pg[kb] = rows(dy).sum(0)
        else:
            zr, mean, invstd = saved[i]
            b = bn_act_bwd(zr, rows(dy), mean, invstd, P[kbn + ".weight"], P[kbn + ".bias"], train)
            pg[kbn + ".weight"], pg[kbn + ".bias"] = b["dgamma"], b["dbeta"]
            dz = unrows(b["dz"], B, Ho, Wo)
            if op.res is not None:
                give(op.res, dy)
        xin = conv_in(op)
        pg[kw], _ = conv_wgrad(r(xin), P[kw].shape, r(dz), st)
        if op.src == "x":
            continue
        dx, _ = conv_dgrad(xin.shape, r(P[kw]), r(dz), st)
        if op.cin_up == 0:
            give(op.src, dx)
        else:
            dlow, _, dtail = upcat_bwd(dx, op.cin_up)
            give(op.src2, dlow)
            give(op.src, dtail)
    return dict(logits=logits, grads=pg, running=running)

