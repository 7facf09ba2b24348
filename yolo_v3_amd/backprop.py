"""Backpropagation of YoloNet's loss into every parameter (reference train.py: ``loss = net(inp, labels); loss.backward()``).

``net.backprop = True`` routes ``net(x, target)`` here.  ``net.backprop_math`` picks the arithmetic of the convolutions (``net.math_mode``
governs inference only): ``F32`` (the default) runs the step in exact fp32 on the kernels of csrc/train.hip; ``BF16`` rounds the two
operands of every convolution product to bf16 (forward: x and w; dgrad: dz and w; wgrad: x and dz) and accumulates in fp32 on the
kernels of csrc/train_bf16.hip, with z, dx and dw in fp32 and everything else exactly as in F32.  The steps below name the F32 calls;
BF16 uses their ``_bf16`` counterparts and keeps a bf16 copy (yv3_train_to_bf16) of each conv input and each dz beside the fp32 one.
``BF16_ACT`` is the BF16 step with every conv_bn_relu activation stored once, in bf16, and no fp32 twin: the conv writes
``zb = bf16(z)`` (yv3_train_conv_fwd_bf16o), the statistics and both BatchNorm passes read zb, the layer output is
``bf16(leaky(bn(zb)) [+ res])`` (yv3_train_bn_act_fwd_bf16), and the BatchNorm / bias backward writes dz as bf16
(yv3_train_bn_act_bwd_bf16, yv3_train_bias_bwd_bf16).  The head logits, dy / dx, parameters, gradients and statistics stay fp32; a
rounding's gradient is the identity.  The steps:

* forward: each conv_bn_relu is ``z = conv(x, w)`` (yv3_train_conv_fwd), the BatchNorm statistics (yv3_train_bn_stats: the batch's
  mean and biased variance in ``.train()``, the running statistics in ``.eval()``) and ``y = leaky(bn(z)) [+ residual]``
  (yv3_train_bn_act_fwd); a head conv is ``z = conv(x, w) + b``; the loss and dL/dlogits come from yv3_yolo_loss;
* backward, in reverse order: dz from dy (yv3_train_bn_act_bwd, or yv3_train_bias_bwd for a head), dw (yv3_train_conv_wgrad)
  and dx (yv3_train_conv_dgrad, plus yv3_train_upcat_bwd after an upsample).  Gradients of activations that fan out -- residual
  skips, the route tails (Darknet layers 36 and 61) and the route heads -- are summed in a fixed order (yv3_train_add).

One ``torch.autograd.Function`` covers the whole network: it takes the input and the parameters (``net.parameters()`` order, i.e.
``state_dict`` order without the buffers) and keeps z, y and the statistics of every layer for the backward.  Backward stops at the
first layer whose inputs need no gradient, e.g. at the backbone/head boundary when the backbone is frozen.  In ``.train()``
the running statistics move as nn.BatchNorm2d moves them (momentum, unbiased variance, ``num_batches_tracked``).

Two Functions share that forward (``net_forward``) and that reverse walk (``walk``).  ``_TrainStep`` is ``net(x, target)``: the loss
comes out, and the walk starts from the loss kernel's dL/dlogits scaled by dL/dloss.  ``_Logits`` is ``net.logits(x)``: the three
heads' logits come out as NCHW views, and the walk starts from whatever gradients autograd hands back for them, so any loss written
in torch on the logits (``net.yoloK(lgK, img_dim, target)`` included) trains the net.

The input gradient is opt-in (``net.input_grad = True``; an ``x`` that requires grad raises NotImplementedError otherwise).  The
walk then runs down to layer 0, whose dgrad (yv3_train_conv0_dgrad) writes dL/dx in x's own NCHW layout, and ``x`` is a real input
of the Function."""
import numbers

import torch
import torch.nn as nn

from . import _ffi
from . import yololayer as _yl


class _Op:
    """One convolution of the net: the conv_bn_relu (or head nn.Conv2d) `module`, reading buffer `src` (and the low-resolution
    `src2`, upsampled and concatenated in front of `src`, when cin_up > 0), writing buffer `out`; `res`: buffer added after the
    activation."""
    __slots__ = ("module", "conv", "bn", "head", "src", "src2", "cin_up", "res", "out", "head_idx")

    def __init__(self, module, src, out, res=None, src2=None, cin_up=0, head_idx=None):
        self.module, self.src, self.out, self.res, self.src2, self.cin_up, self.head_idx = module, src, out, res, src2, cin_up, head_idx
        self.head = isinstance(module, nn.Conv2d)
        self.conv = module if self.head else module.conv
        self.bn = None if self.head else module.bn


def graph(net):
    """The net as a list of _Op in execution order (reference darknet.py:198-231)."""
    from .darknet import res_layer
    ops = []
    feat = net.feature.mlist
    ops.append(_Op(feat[0], "x", "f0"))
    cur = "f0"
    for pos in range(1, len(feat)):
        m = feat[pos]
        if isinstance(m, res_layer):
            ops.append(_Op(m.conv1, cur, "f%da" % pos))
            ops.append(_Op(m.conv2, "f%da" % pos, "f%d" % pos, res=cur))
        else:
            ops.append(_Op(m, cur, "f%d" % pos))
        cur = "f%d" % pos
    r61, r36 = "f%d" % net.feature.map2yolocfg[61], "f%d" % net.feature.map2yolocfg[36]

    def predet(group, name, src, k, src2=None, cin_up=0):
        prev = src
        for i, m in enumerate(group.mlist[:-1]):
            out = "%s.%d" % (name, i)
            ops.append(_Op(m, prev, out, src2=src2 if i == 0 else None, cin_up=cin_up if i == 0 else 0))
            prev = out
        ops.append(_Op(group.mlist[-1], prev, "%s.logits" % name, head_idx=k))
        return "%s.%d" % (name, group.getIdxFromYoloIdx(-3))

    h1 = predet(net.pre_det1, "pre_det1", cur, 0)
    ops.append(_Op(net.up1.conv, h1, "up1"))
    h2 = predet(net.pre_det2, "pre_det2", r61, 1, src2="up1", cin_up=net.up1.conv.conv.out_channels)
    ops.append(_Op(net.up2.conv, h2, "up2"))
    predet(net.pre_det3, "pre_det3", r36, 2, src2="up2", cin_up=net.up2.conv.conv.out_channels)
    return ops


def _f32(t, what):
    _ffi.require_cuda(t, what)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _ffi.Yv3Error("%s must be a contiguous fp32 tensor for the training path" % what)
    return t.detach()


def _round8(c):
    return (c + 7) & ~7


def backprop_math(net):
    """net.backprop_math, checked: F32, BF16 or BF16_ACT, else Yv3Error (YV3_EINVAL)."""
    m = getattr(net, "backprop_math", _ffi.F32)
    if not isinstance(m, numbers.Integral) or isinstance(m, bool) or m not in (_ffi.F32, _ffi.BF16, _ffi.BF16_ACT):
        err = _ffi.Yv3Error("net.backprop_math must be yolo_v3_amd.F32, yolo_v3_amd.BF16 or yolo_v3_amd.BF16_ACT, got %r" % (m,))
        err.code = _ffi.EINVAL
        raise err
    return int(m)


def _bf16(lib, s, t, rows, C, ld, what):
    """A bf16 copy (int16 storage) of the fp32 tensor t seen as rows x C, padded with zero channels to ld."""
    out = torch.empty(rows * ld, device=t.device, dtype=torch.int16)
    _ffi.check(lib.yv3_train_to_bf16(t.data_ptr(), out.data_ptr(), rows, C, ld, s), "yv3_train_to_bf16 (%s)" % what)
    return out


class _Run:
    """Forward state of one training step: what the backward needs."""

    def __init__(self, net, x, target, math=_ffi.F32, input_grad=False):
        self.net, self.x, self.target, self.math, self.input_grad = net, x, target, math, bool(input_grad)
        self.ops = graph(net)
        self.saved = {}            # op index -> dict of tensors
        self.shape = {}            # buffer -> (B, H, W, C)
        self.need = {}             # buffer -> some parameter upstream of it needs a gradient
        self.loss = None
        # None: nothing extra.  A dict: backward() stores, per op index, clones of dy, dz, the parameter gradients and every
        # destination of a dgrad / upcat_bwd / add before and after the call (tests/test_gpu_train_local.py checks each op on them)
        self.trace = None


def _ws(nbytes, dev):
    if nbytes == 0:
        raise _ffi.Yv3Error("training kernel shape out of range")
    return torch.empty(nbytes, device=dev, dtype=torch.uint8)


def net_forward(run, want_grad):
    """The training forward of the whole net up to the heads -> their logits [(fp32 NHWC tensor, h, w)] * 3; with want_grad the
    run keeps what the walk needs."""
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    net, x = run.net, run.x
    B, _, H, W = x.shape
    dev = x.device
    bufs = {"x": x}
    act = run.math == _ffi.BF16_ACT            # activations in bf16 only: bufs holds x and the head logits, bufs_b the rest
    bf = act or run.math == _ffi.BF16
    bufs_b = {"x": _bf16(lib, s, x, x.numel(), 1, 1, "x")} if bf else None      # bf16 conv inputs (BF16: copies of bufs' tensors)
    last = {}                                  # buffer -> index of the last op that reads it in the forward
    for i, op in enumerate(run.ops):
        last.update({b: i for b in (op.src, op.src2, op.res) if b is not None})
    keep = set()                               # BF16_ACT: the bf16 buffers the walk reads (the inputs of a wgrad)
    run.shape["x"] = (B, H, W, 3)
    run.need["x"] = run.input_grad
    logits = [None] * 3
    for i, op in enumerate(run.ops):
        c = op.conv
        cin, cout, k, st = c.in_channels, c.out_channels, c.kernel_size[0], c.stride[0]
        b_, h, w, ct = run.shape[op.src]
        if ct + op.cin_up != cin:
            raise _ffi.Yv3Error("%s: %d input channels, expected %d" % (op.out, ct + op.cin_up, cin))
        ho, wo = (h + 2 * ((k - 1) // 2) - k) // st + 1, (w + 2 * ((k - 1) // 2) - k) // st + 1
        wt = _f32(c.weight, "weight of " + op.out)
        params = [c.weight] + ([c.bias] if op.head else [op.bn.weight, op.bn.bias])
        run.need[op.out] = any(p.requires_grad for p in params) or run.need[op.src] or \
            (op.src2 is not None and run.need[op.src2]) or (op.res is not None and run.need[op.res])
        sv = {}
        if want_grad and c.weight.requires_grad:
            keep.update(b for b in (op.src, op.src2) if b is not None)
        zb16 = act and not op.head
        z = torch.empty((b_, ho, wo, cout), device=dev, dtype=torch.int16 if zb16 else torch.float32)
        bias = _f32(c.bias, "bias of " + op.out) if op.head else None
        if bf:
            wf = torch.empty(_round8(cout) * cin * k * k, device=dev, dtype=torch.int16)
            wd = torch.empty_like(wf) if want_grad else None
            _ffi.check(lib.yv3_train_pack_weight_bf16(wt.data_ptr(), wf.data_ptr(), wd.data_ptr() if wd is not None else None,
                                                      cout, cin, k, s), "yv3_train_pack_weight_bf16")
            x2 = bufs_b[op.src2] if op.src2 is not None else None
            if zb16:
                _ffi.check(lib.yv3_train_conv_fwd_bf16o(bufs_b[op.src].data_ptr(), x2.data_ptr() if x2 is not None else None,
                                                        wf.data_ptr(), z.data_ptr(), b_, h, w, cin, op.cin_up, cout, k, st,
                                                        int(op.src == "x"), s), "yv3_train_conv_fwd_bf16o")
            else:
                _ffi.check(lib.yv3_train_conv_fwd_bf16(bufs_b[op.src].data_ptr(), x2.data_ptr() if x2 is not None else None,
                                                       wf.data_ptr(), bias.data_ptr() if bias is not None else None, z.data_ptr(),
                                                       b_, h, w, cin, op.cin_up, cout, k, st, int(op.src == "x"), s),
                           "yv3_train_conv_fwd_bf16")
        else:
            wf = torch.empty(cout * cin * k * k, device=dev, dtype=torch.float32)
            wd = torch.empty_like(wf) if want_grad else None
            _ffi.check(lib.yv3_train_pack_weight(wt.data_ptr(), wf.data_ptr(), wd.data_ptr() if wd is not None else None,
                                                 cout, cin, k, s), "yv3_train_pack_weight")
            x2 = bufs[op.src2] if op.src2 is not None else None
            _ffi.check(lib.yv3_train_conv_fwd(bufs[op.src].data_ptr(), x2.data_ptr() if x2 is not None else None, wf.data_ptr(),
                                              bias.data_ptr() if bias is not None else None, z.data_ptr(), b_, h, w, cin, op.cin_up,
                                              cout, k, st, int(op.src == "x"), s), "yv3_train_conv_fwd")
        run.shape[op.out] = (b_, ho, wo, cout)
        sv.update(wd=wd, geo=(b_, h, w, cin, cout, k, st))
        if op.head:
            bufs[op.out] = z
            logits[op.head_idx] = (z, ho, wo)
        else:
            bn = op.bn
            P = b_ * ho * wo
            mean = torch.empty(cout, device=dev, dtype=torch.float32)
            invstd = torch.empty_like(mean)
            g, bt = _f32(bn.weight, "bn.weight of " + op.out), _f32(bn.bias, "bn.bias of " + op.out)
            if bn.training:
                rm, rv = _f32(bn.running_mean, "running_mean"), _f32(bn.running_var, "running_var")
                with torch.no_grad():
                    bn.num_batches_tracked.add_(1)
                mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                rm_new, rv_new = torch.empty_like(rm), torch.empty_like(rv)
                nb = (lib.yv3_train_channel_bf16_workspace_bytes if act else lib.yv3_train_channel_workspace_bytes)(P, cout)
                ws = _ws(nb, dev)
                stats = lib.yv3_train_bn_stats_bf16 if act else lib.yv3_train_bn_stats
                _ffi.check(stats(z.data_ptr(), P, cout, float(bn.eps), float(mom), rm.data_ptr(), rv.data_ptr(),
                                 rm_new.data_ptr(), rv_new.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), nb, s),
                           "yv3_train_bn_stats")
                with torch.no_grad():          # (copy_ moves the buffers' _version: the inference engine re-packs)
                    bn.running_mean.copy_(rm_new)
                    bn.running_var.copy_(rv_new)
            else:
                _ffi.check(lib.yv3_train_bn_eval_stats(bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(bn.eps),
                                                       mean.data_ptr(), invstd.data_ptr(), cout, s), "yv3_train_bn_eval_stats")
            y = torch.empty_like(z)
            res = (bufs_b if act else bufs)[op.res] if op.res is not None else None
            _ffi.check((lib.yv3_train_bn_act_fwd_bf16 if act else lib.yv3_train_bn_act_fwd)(
                z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), g.data_ptr(), bt.data_ptr(),
                res.data_ptr() if res is not None else None, y.data_ptr(), P, cout, s), "yv3_train_bn_act_fwd")
            if act:
                bufs_b[op.out] = y
                if not (want_grad and run.need[op.out]):       # no walk will reach this op
                    z = None
            else:
                bufs[op.out] = y
                if bf:                         # (every conv_bn_relu output is some conv's input)
                    bufs_b[op.out] = _bf16(lib, s, y, P, cout, cout, op.out)
            sv.update(z=z, mean=mean, invstd=invstd, gamma=g, beta=bt, train=int(bn.training))
        run.saved[i] = sv
        if act:                                # a bf16 buffer lives until its last reader: a later op, or a wgrad of the walk
            for b in {op.src, op.src2, op.res} - {None}:
                if last[b] == i and b not in keep:
                    del bufs_b[b]
    if want_grad:
        run.bufs = bufs
        run.bufs_b = bufs_b
    return logits


def forward(run, want_grad):
    """The training forward of the whole net, the loss and dL/dlogits; returns the loss (fp32 0-d GPU tensor) and sets net.stats."""
    net, x = run.net, run.x
    B, H, dev = x.shape[0], x.shape[2], x.device
    logits = net_forward(run, want_grad)
    # the loss of the three heads (as YoloNet._loss), with dL/dlogits when a backward will follow
    heads = (net.yolo1, net.yolo2, net.yolo3)
    t = _yl.loss_target(run.target, B, dev)
    out = torch.empty(3 * _yl.HEAD_OUT_BYTES, device=dev, dtype=torch.uint8)
    run.dlogits = []
    for kk, ((lg, hh, ww), head) in enumerate(zip(logits, heads)):
        ld = lg.shape[-1]
        gr = torch.empty_like(lg) if want_grad else None
        _yl.launch_loss(lg, (hh * ww * ld, ld, 1), t, hh, ww, net.numClass, H, head.anchors_all, head.anchors_mask,
                        out[kk * _yl.HEAD_OUT_BYTES:], gr)
        run.dlogits.append(gr)
    return net._loss_from_device(out, B, dev)


def walk(run, dlogits, scale=None):
    """The reverse walk from the heads: dlogits[k] = dL/dlogits of head k (contiguous NHWC fp32, or None: that head got no gradient),
    times the fp32 0-d GPU tensor `scale` when one is given.  -> ({id(param): dL/dparam}, dL/dx [B,3,H,W] fp32 or None); the
    latter when run.need["x"]."""
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    dev = run.x.device
    act = run.math == _ffi.BF16_ACT
    bf = act or run.math == _ffi.BF16
    grads = {}                 # buffer -> dL/dbuffer (NHWC fp32; "x": NCHW)
    pg = {}
    trace = run.trace

    def rec(i, **tensors):
        if trace is not None:
            trace.setdefault(i, {}).update({k: t.clone() for k, t in tensors.items() if t is not None})

    def give(i, buf, t):
        """Add t into the gradient of buf (takes ownership of t when buf has none yet)."""
        if buf in grads:
            rec(i, res_before=grads[buf])
            _ffi.check(lib.yv3_train_add(t.data_ptr(), grads[buf].data_ptr(), t.numel(), s), "yv3_train_add")
        else:
            grads[buf] = t
        rec(i, res_after=grads[buf])

    head_ops = {op.head_idx: op for op in run.ops if op.head}
    for kk in range(3):
        if dlogits[kk] is not None:
            grads[head_ops[kk].out] = dlogits[kk]
    for i in range(len(run.ops) - 1, -1, -1):
        op, sv = run.ops[i], run.saved[i]
        dy = grads.pop(op.out, None)
        if dy is None or not run.need[op.out]:
            continue
        rec(i, dy=dy)
        b_, h, w, cin, cout, k, st = sv["geo"]
        _, ho, wo, _ = run.shape[op.out]
        P = b_ * ho * wo
        nb = (lib.yv3_train_channel_bf16_workspace_bytes if act else lib.yv3_train_channel_workspace_bytes)(P, cout)
        ws = _ws(nb, dev)
        # BF16_ACT: dz is born in bf16, in the padded rows the dgrad / wgrad kernels read
        dz = torch.empty(P * _round8(cout), device=dev, dtype=torch.int16) if act else torch.empty_like(dy)
        c = op.conv
        if op.head:
            db = torch.empty(cout, device=dev, dtype=torch.float32)
            _ffi.check((lib.yv3_train_bias_bwd_bf16 if act else lib.yv3_train_bias_bwd)(
                dy.data_ptr(), scale.data_ptr() if scale is not None else None, dz.data_ptr(), db.data_ptr(), P, cout, ws.data_ptr(),
                nb, s), "yv3_train_bias_bwd")
            pg[id(c.bias)] = db
            rec(i, dz=dz, dbias=db)
        else:
            dgam = torch.empty(cout, device=dev, dtype=torch.float32)
            dbet = torch.empty_like(dgam)
            _ffi.check((lib.yv3_train_bn_act_bwd_bf16 if act else lib.yv3_train_bn_act_bwd)(
                sv["z"].data_ptr(), dy.data_ptr(), sv["mean"].data_ptr(), sv["invstd"].data_ptr(), sv["gamma"].data_ptr(),
                sv["beta"].data_ptr(), dz.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), P, cout, sv["train"], ws.data_ptr(), nb, s),
                "yv3_train_bn_act_bwd")
            pg[id(op.bn.weight)], pg[id(op.bn.bias)] = dgam, dbet
            rec(i, dz=dz, dgamma=dgam, dbeta=dbet)
            if op.res is not None and run.need[op.res]:
                give(i, op.res, dy)         # y = act(...) + res: dres = dy (dy is not read again)
        need_src = run.need[op.src]
        need_src2 = op.src2 is not None and run.need[op.src2]
        if bf:
            dzb = dz if act else _bf16(lib, s, dz, P, cout, _round8(cout), "dz of " + op.out)
        if c.weight.requires_grad:
            dw = torch.empty_like(c.weight, dtype=torch.float32, memory_format=torch.contiguous_format)
            if bf:
                nw = lib.yv3_train_conv_wgrad_bf16_workspace_bytes(b_, h, w, cin, cout, k, st)
                wsw = _ws(nw, dev)
                x2 = run.bufs_b[op.src2] if op.src2 is not None else None
                _ffi.check(lib.yv3_train_conv_wgrad_bf16(run.bufs_b[op.src].data_ptr(), x2.data_ptr() if x2 is not None else None,
                                                         dzb.data_ptr(), dw.data_ptr(), b_, h, w, cin, op.cin_up, cout, k, st,
                                                         int(op.src == "x"), wsw.data_ptr(), nw, s), "yv3_train_conv_wgrad_bf16")
            else:
                nw = lib.yv3_train_conv_wgrad_workspace_bytes(b_, h, w, cin, cout, k, st)
                wsw = _ws(nw, dev)
                x2 = run.bufs[op.src2] if op.src2 is not None else None
                _ffi.check(lib.yv3_train_conv_wgrad(run.bufs[op.src].data_ptr(), x2.data_ptr() if x2 is not None else None,
                                                    dz.data_ptr(), dw.data_ptr(), b_, h, w, cin, op.cin_up, cout, k, st,
                                                    int(op.src == "x"), wsw.data_ptr(), nw, s), "yv3_train_conv_wgrad")
            pg[id(c.weight)] = dw
            rec(i, dw=dw)
        if not (need_src or need_src2):
            continue
        if op.src == "x":                  # layer 0: dL/dx in the caller's NCHW layout, from the parameter itself
            dx = torch.empty((b_, cin, h, w), device=dev, dtype=torch.float32)
            wt = _f32(c.weight, "weight of " + op.out)
            if bf:
                _ffi.check(lib.yv3_train_conv0_dgrad_bf16(dzb.data_ptr(), wt.data_ptr(), dx.data_ptr(), b_, h, w, cout, s),
                           "yv3_train_conv0_dgrad_bf16")
            else:
                _ffi.check(lib.yv3_train_conv0_dgrad(dz.data_ptr(), wt.data_ptr(), dx.data_ptr(), b_, h, w, cout, s),
                           "yv3_train_conv0_dgrad")
            grads["x"] = dx
            rec(i, dx_after=dx)
            continue

        def dgrad(dx, acc):
            if bf:
                _ffi.check(lib.yv3_train_conv_dgrad_bf16(dzb.data_ptr(), sv["wd"].data_ptr(), dx.data_ptr(), b_, h, w, cin, cout, k, st,
                                                         int(acc), s), "yv3_train_conv_dgrad_bf16")
            else:
                _ffi.check(lib.yv3_train_conv_dgrad(dz.data_ptr(), sv["wd"].data_ptr(), dx.data_ptr(), b_, h, w, cin, cout, k, st,
                                                    int(acc), s), "yv3_train_conv_dgrad")

        if op.cin_up == 0:
            acc = op.src in grads
            dx = grads[op.src] if acc else torch.empty((b_, h, w, cin), device=dev, dtype=torch.float32)
            rec(i, dx_before=dx if acc else None)
            dgrad(dx, acc)
            grads[op.src] = dx
            rec(i, dx_after=dx)
        else:
            dcat = torch.empty((b_, h, w, cin), device=dev, dtype=torch.float32)
            dgrad(dcat, False)
            ct = cin - op.cin_up
            dlow = dtail = None
            acc_low = acc_tail = 0
            if need_src2:
                acc_low = int(op.src2 in grads)
                dlow = grads[op.src2] if acc_low else torch.empty((b_, h // 2, w // 2, op.cin_up), device=dev, dtype=torch.float32)
                grads[op.src2] = dlow
            if need_src:
                acc_tail = int(op.src in grads)
                dtail = grads[op.src] if acc_tail else torch.empty((b_, h, w, ct), device=dev, dtype=torch.float32)
                grads[op.src] = dtail
            rec(i, dcat=dcat, dlow_before=dlow if acc_low else None, dtail_before=dtail if acc_tail else None)
            _ffi.check(lib.yv3_train_upcat_bwd(dcat.data_ptr(), dlow.data_ptr() if dlow is not None else None,
                                               dtail.data_ptr() if dtail is not None else None, b_, h, w, op.cin_up, ct,
                                               acc_low, acc_tail, s), "yv3_train_upcat_bwd")
            rec(i, dlow_after=dlow, dtail_after=dtail)
    return pg, grads.get("x")


def loss_walk(run, grad_output):
    """walk() from the loss kernel's dL/dlogits (forward(run, want_grad=True)) for dL/dloss = grad_output."""
    g = grad_output.detach().to(device=run.x.device, dtype=torch.float32).reshape(()).contiguous()
    return walk(run, run.dlogits, g)


def backward(run, grad_output):
    """dL/dparameter for every parameter that requires grad, as {id(param): tensor}, for dL/dloss = grad_output."""
    return loss_walk(run, grad_output)[0]


def _input_grads(ctx, x, params, pg, dx):
    """The backward's return values for (run, x, *params)."""
    out = []
    for i, p in enumerate(params):
        gp = pg.get(id(p)) if ctx.needs_input_grad[2 + i] else None
        out.append(gp.view_as(p) if gp is not None else None)
    gx = dx.to(x.dtype) if dx is not None and ctx.needs_input_grad[1] else None
    return (None, gx) + tuple(out)


class _TrainStep(torch.autograd.Function):
    """loss = YoloNet(x, target) in training form; backward fills the parameters' gradients (one Function for the whole net)."""

    @staticmethod
    def forward(ctx, run, x, *params):
        loss = forward(run, want_grad=True)
        ctx.run = run
        ctx.save_for_backward(x, *params)      # (an in-place change of a parameter before backward() then raises, as in torch)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        x, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        run = ctx.run
        ctx.run = None
        with torch.cuda.device(run.x.device):
            pg, dx = loss_walk(run, grad_output)
        return _input_grads(ctx, x, params, pg, dx)


class _Logits(torch.autograd.Function):
    """(lg1, lg2, lg3) = the heads' logits of YoloNet(x) in training form, as NCHW views; backward walks the net from the gradients
    autograd hands back for them (any strides; a head that got none counts as zero)."""

    @staticmethod
    def forward(ctx, run, x, *params):
        logits = net_forward(run, want_grad=True)
        ctx.run = run
        ctx.save_for_backward(x, *params)
        ctx.set_materialize_grads(False)
        return tuple(z.permute(0, 3, 1, 2) for z, _, _ in logits)

    @staticmethod
    def backward(ctx, *grad_logits):
        x, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        run = ctx.run
        ctx.run = None
        dev = run.x.device
        with torch.cuda.device(dev):
            dl = [None if g is None else g.detach().to(device=dev, dtype=torch.float32).permute(0, 2, 3, 1).contiguous()
                  for g in grad_logits]
            pg, dx = walk(run, dl)
        return _input_grads(ctx, x, params, pg, dx)


def _start(net, x, target):
    """The checks of the training path -> (the Function's x argument, the run, the parameters, differentiable?)."""
    math = backprop_math(net)
    if not x.is_cuda:
        raise _ffi.GpuOnlyError("input images must live on the GPU: this package runs only on MI355X (HIP kernels), "
                                "there is no CPU path")
    input_grad = bool(getattr(net, "input_grad", False))
    if x.requires_grad and not input_grad:
        raise NotImplementedError("the training path computes the input gradient only with net.input_grad = True: set it, or pass "
                                  "x without requires_grad")
    if x.dim() != 4 or x.shape[1] != 3:
        raise _ffi.Yv3Error("input must be [B, 3, H, W], got %s" % (tuple(x.shape),))
    if x.shape[2] % 32 or x.shape[3] % 32:
        raise _ffi.Yv3Error("input height and width must be multiples of 32, got %dx%d" % (x.shape[2], x.shape[3]))
    params = list(net.parameters())
    want_x = x.requires_grad and torch.is_grad_enabled()
    run = _Run(net, x.detach().float().contiguous(), target, math, input_grad=want_x)
    diff = torch.is_grad_enabled() and (want_x or any(p.requires_grad for p in params))
    return (x if want_x else run.x), run, params, diff


def loss(net, x, target):
    """net(x, target) with net.backprop = True (see the module docstring)."""
    x, run, params, diff = _start(net, x, target)
    with torch.cuda.device(run.x.device):
        if diff:
            return _TrainStep.apply(run, x, *params)
        with torch.no_grad():
            return forward(run, want_grad=False)


def logits(net, x):
    """net.logits(x): the three heads' logits (lg1, lg2, lg3), each [B, 3*(5+C), h, w] (NCHW views of the fp32 NHWC buffers), from
    the training forward -- BatchNorm in the module's mode, arithmetic by net.backprop_math -- differentiable in the parameters and,
    with net.input_grad, in x (see the module docstring).  Under torch.no_grad(), or when nothing requires grad, forward only."""
    x, run, params, diff = _start(net, x, None)
    with torch.cuda.device(run.x.device):
        if diff:
            return _Logits.apply(run, x, *params)
        with torch.no_grad():
            return tuple(z.permute(0, 3, 1, 2) for z, _, _ in net_forward(run, want_grad=False))
