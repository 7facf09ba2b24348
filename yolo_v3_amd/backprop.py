"""Backpropagation of YoloNet's loss into every parameter (reference train.py: ``loss = net(inp, labels); loss.backward()``).

``net.backprop = True`` routes ``net(x, target)`` here.  ``net.backprop_math`` picks the arithmetic of the step (``net.math_mode``
governs inference only).  ``MATH`` holds one record per value: the library entry points the step calls, by name, and the few facts
about its buffers that differ; ``net_forward`` and ``walk`` call every kernel from one place, through the record.  ``F32`` (the
default) is exact fp32 on the kernels of csrc/train.hip.  ``BF16`` rounds the two operands of every convolution product to bf16
(forward: x and w; dgrad: dz and w; wgrad: x and dz) and accumulates in fp32 on the kernels of csrc/train_bf16.hip; z, dx and dw
are fp32 and everything else is F32's; the bf16 operands are copies (yv3_train_to_bf16) of each conv input and each dz beside the
fp32 ones.  ``BF16_ACT`` is the BF16 step with every conv_bn_relu activation stored once, in bf16, and no fp32 twin: the conv writes
``zb = bf16(z)``, the statistics and both BatchNorm passes read zb, the layer output is ``bf16(leaky(bn(zb)) [+ res])``, and the
BatchNorm / bias backward writes dz as bf16 (csrc/train_bf16_act.hip).  The head logits, dy / dx, parameters, gradients and
statistics stay fp32; a rounding's gradient is the identity.  The steps, by the record's fields:

* forward: each conv_bn_relu is ``z = conv(x, w)`` (pack_weight, conv_fwd), the BatchNorm statistics (bn_stats: the batch's
  mean and biased variance in ``.train()``; yv3_train_bn_eval_stats: the running statistics in ``.eval()``) and
  ``y = leaky(bn(z)) [+ residual]`` (bn_act_fwd); a head conv is ``z = conv(x, w) + b`` (conv_fwd_head); the loss and dL/dlogits
  come from yv3_yolo_loss;
* backward, in reverse order: dz from dy (bn_act_bwd, or bias_bwd for a head), dw (conv_wgrad) and dx (conv_dgrad, plus
  yv3_train_upcat_bwd after an upsample).  Gradients of activations that fan out -- residual skips, the route tails (Darknet
  layers 36 and 61) and the route heads -- are summed in a fixed order (yv3_train_add).

One ``torch.autograd.Function`` covers the whole network: it takes the input and the parameters (``net.parameters()`` order, i.e.
``state_dict`` order without the buffers) and keeps z, y and the statistics of every layer for the backward.  Backward stops at the
first layer whose inputs need no gradient, e.g. at the backbone/head boundary when the backbone is frozen.  In ``.train()``
the running statistics move as nn.BatchNorm2d moves them (momentum, unbiased variance, ``num_batches_tracked``).

Two Functions share that forward (``net_forward``) and that reverse walk (``walk``).  ``_TrainStep`` is ``net(x, target)``: the loss
comes out, and the walk starts from the loss kernel's dL/dlogits scaled by dL/dloss.  ``_Logits`` is ``net.logits(x)``: the three
heads' logits come out as NCHW views, and the walk starts from whatever gradients autograd hands back for them, so any loss written
in torch on the logits (``net.yoloK(lgK, img_dim, target)`` included) trains the net.

The input gradient is opt-in (``net.input_grad = True``; an ``x`` that requires grad raises NotImplementedError otherwise).  The
walk then runs down to layer 0, whose dgrad (conv0_dgrad) writes dL/dx in x's own NCHW layout, and ``x`` is a real input
of the Function.

``net.frozen_prefix = True`` (opt-in) runs the frozen eval-mode prefix of the net -- ``frozen_prefix_ops(net)`` leading ops, e.g. the
52 of a frozen ``net.feature.eval()`` -- on the inference engine instead: a prefix engine (engine.Engine with n_conv) in the exact F32
plan for F32 and in the BF16 plan for BF16 / BF16_ACT, whose outputs are copied into the run's buffers where a later op reads them
(``_prefix``).  Everything from the first trainable or train-mode op on, the walk included, is as without the switch."""
import functools
import numbers
from collections import namedtuple

import torch
import torch.nn as nn

from . import _ffi, arch
from . import engine as _engine
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


def _buffer(sp):
    """The run's name for the output of the conv of spec sp: feature.mlist.<pos>[.conv2] -> f<pos> (.conv1: f<pos>a), upK.conv -> upK,
    pre_detK.mlist.<i> -> pre_detK.<i> (the head conv: pre_detK.logits).  The input image is "x"."""
    part = sp.name.split(".")
    if part[0] == "feature":
        return "f" + part[2] + ("a" if part[-1] == "conv1" else "")
    if not sp.bn:
        return part[0] + ".logits"
    return part[0] if part[-1] == "conv" else "%s.%s" % (part[0], part[2])


@functools.lru_cache(maxsize=1)
def _ops():
    """Per conv of arch.wiring: (the module's path from the net, _Op's arguments after the module); the same for every net."""
    specs = arch.conv_specs()
    out = []
    for sp, wr in zip(specs, arch.wiring(specs)):
        x, x2, res = (None if j is None else _buffer(specs[j]) for j in (wr.x, wr.x2, wr.residual))
        x = x or "x"
        src, src2 = (x, None) if x2 is None else (x2, x)      # _Op.src is the full-resolution input: at a join the route, Wire.x2
        out.append((sp.name.split("."), (src, _buffer(sp), res, src2, wr.cin_up, wr.head)))
    return out


def graph(net):
    """The net as a list of _Op in execution order (arch.wiring; reference darknet.py:198-231)."""
    ops = []
    for path, args in _ops():
        m = net
        for part in path:                # (straight from the modules' dicts: nn.Module.__getattr__ and get_submodule are slow)
            m = m._modules[part]
        ops.append(_Op(m, *args))
    return ops


FRONT_OPS = _engine.Engine.FRONT_CONVS     # the ops the inference plans run as the fused front: no prefix is shorter
PREFIX_MODE = {_ffi.F32: _ffi.F32, _ffi.BF16: _ffi.BF16, _ffi.BF16_ACT: _ffi.BF16}      # net.backprop_math -> the prefix's inference mode


def frozen_prefix_ops(net, input_grad=False):
    """The number of leading ops of graph(net) that a training step may run on the inference engine (``net.frozen_prefix``): the
    longest leading run in which no parameter requires grad and every BatchNorm is in eval mode -- there the training forward
    computes what the inference engine computes, eval-mode BatchNorm folded into the conv epilogue, and no backward reaches it.  A
    frozen head conv may be part of it.  0 when the input needs a gradient (`input_grad`), and when the run is shorter than the
    fused front (FRONT_OPS), whose inner buffers the plans never write."""
    return _prefix_len(graph(net), input_grad)


def _prefix_len(ops, input_grad):
    if input_grad:
        return 0
    n = 0
    for op in ops:
        c = op.conv
        params = [c.weight, c.bias] if op.head else [c.weight, op.bn.weight, op.bn.bias]
        if any(p.requires_grad for p in params) or (op.bn is not None and op.bn.training):
            break
        n += 1
    return n if n >= FRONT_OPS else 0


def _f32(t, what):
    _ffi.require_cuda(t, what)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _ffi.Yv3Error("%s must be a contiguous fp32 tensor for the training path" % what)
    return t.detach()


def _round8(c):
    return (c + 7) & ~7


# What one net.backprop_math value fixes.  ENTRIES name the library's entry points: the weight pack, the conv forward of a
# conv_bn_relu and of a head, dgrad, layer 0's dgrad, wgrad and its workspace query, the per-channel kernels' workspace query and
# those kernels.  The facts: act_dtype, how a conv_bn_relu's z and output are stored (int16: as bf16 only, in bufs_b); bf16_operands,
# whether the convs read bf16 tensors (run.bufs_b) or the fp32 ones (run.bufs); cast_twins, whether those are cast copies
# (yv3_train_to_bf16) of each fp32 output and dz -- without it they are born in bf16; pad, cout -> the channels of a dz row and of a
# packed weight's outputs.
_Math = namedtuple("_Math", "pack_weight conv_fwd conv_fwd_head conv_dgrad conv0_dgrad conv_wgrad conv_wgrad_ws channel_ws bn_stats "
                            "bn_act_fwd bn_act_bwd bias_bwd act_dtype bf16_operands cast_twins pad")
ENTRIES = _Math._fields[:12]
MATH = {_ffi.F32: _Math(                     # net.backprop_math -> its _Math
    pack_weight="yv3_train_pack_weight", conv_fwd="yv3_train_conv_fwd", conv_fwd_head="yv3_train_conv_fwd",
    conv_dgrad="yv3_train_conv_dgrad", conv0_dgrad="yv3_train_conv0_dgrad", conv_wgrad="yv3_train_conv_wgrad",
    conv_wgrad_ws="yv3_train_conv_wgrad_workspace_bytes", channel_ws="yv3_train_channel_workspace_bytes",
    bn_stats="yv3_train_bn_stats", bn_act_fwd="yv3_train_bn_act_fwd", bn_act_bwd="yv3_train_bn_act_bwd", bias_bwd="yv3_train_bias_bwd",
    act_dtype=torch.float32, bf16_operands=False, cast_twins=False, pad=int)}
MATH[_ffi.BF16] = MATH[_ffi.F32]._replace(
    pack_weight="yv3_train_pack_weight_bf16", conv_fwd="yv3_train_conv_fwd_bf16", conv_fwd_head="yv3_train_conv_fwd_bf16",
    conv_dgrad="yv3_train_conv_dgrad_bf16", conv0_dgrad="yv3_train_conv0_dgrad_bf16", conv_wgrad="yv3_train_conv_wgrad_bf16",
    conv_wgrad_ws="yv3_train_conv_wgrad_bf16_workspace_bytes", bf16_operands=True, cast_twins=True, pad=_round8)
MATH[_ffi.BF16_ACT] = MATH[_ffi.BF16]._replace(
    conv_fwd="yv3_train_conv_fwd_bf16o", channel_ws="yv3_train_channel_bf16_workspace_bytes", bn_stats="yv3_train_bn_stats_bf16",
    bn_act_fwd="yv3_train_bn_act_fwd_bf16", bn_act_bwd="yv3_train_bn_act_bwd_bf16", bias_bwd="yv3_train_bias_bwd_bf16",
    act_dtype=torch.int16, cast_twins=False)
# an entry point whose arguments differ from its field's other entries, brought to their form (a conv_bn_relu has no bias)
_ADAPT = {"yv3_train_conv_fwd_bf16o": lambda f: lambda x, x2, wf, bias, zb, *shape: f(x, x2, wf, zb, *shape)}


def entry(lib, name):
    """The library function behind an entry point of a _Math, taking the arguments of its field."""
    return _ADAPT.get(name, lambda f: f)(getattr(lib, name))


def _call(lib, name, *args, what=None):
    _ffi.check(entry(lib, name)(*args), what or name)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def backprop_math(net):
    """net.backprop_math, checked: F32, BF16 or BF16_ACT, else Yv3Error (YV3_EINVAL)."""
    m = getattr(net, "backprop_math", _ffi.F32)
    if not isinstance(m, numbers.Integral) or isinstance(m, bool) or m not in MATH:
        err = _ffi.Yv3Error("net.backprop_math must be yolo_v3_amd.F32, yolo_v3_amd.BF16 or yolo_v3_amd.BF16_ACT, got %r" % (m,))
        err.code = _ffi.EINVAL
        raise err
    return int(m)


def _bf16(lib, s, t, rows, C, ld, what):
    """A bf16 copy (int16 storage) of the fp32 tensor t seen as rows x C, padded with zero channels to ld."""
    out = torch.empty(rows * ld, device=t.device, dtype=torch.int16)
    _call(lib, "yv3_train_to_bf16", t.data_ptr(), out.data_ptr(), rows, C, ld, s, what="yv3_train_to_bf16 (%s)" % what)
    return out


class _Run:
    """Forward state of one training step: what the backward needs."""

    def __init__(self, net, x, target, math=_ffi.F32, input_grad=False):
        self.net, self.x, self.target, self.math, self.input_grad = net, x, target, math, bool(input_grad)
        self.ops = graph(net)
        # ops [0, prefix) run on the inference engine (net.frozen_prefix): they get a shape, need = False and no `saved` entry
        self.prefix = _prefix_len(self.ops, self.input_grad) if getattr(net, "frozen_prefix", False) else 0
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


def _conv(lib, s, m, run, op, src, want_grad):
    """z = conv(x, w) [+ bias] of one op on the conv operands `src` (bufs or bufs_b) -> (z, what the walk keeps of it)."""
    c = op.conv
    cin, cout, k, st = c.in_channels, c.out_channels, c.kernel_size[0], c.stride[0]
    b_, h, w, ct = run.shape[op.src]
    if ct + op.cin_up != cin:
        raise _ffi.Yv3Error("%s: %d input channels, expected %d" % (op.out, ct + op.cin_up, cin))
    ho, wo = (h + 2 * ((k - 1) // 2) - k) // st + 1, (w + 2 * ((k - 1) // 2) - k) // st + 1
    wt, dev = _f32(c.weight, "weight of " + op.out), run.x.device
    z = torch.empty((b_, ho, wo, cout), device=dev, dtype=torch.float32 if op.head else m.act_dtype)
    bias = _f32(c.bias, "bias of " + op.out) if op.head else None
    wf = torch.empty(m.pad(cout) * cin * k * k, device=dev, dtype=torch.int16 if m.bf16_operands else torch.float32)
    wd = torch.empty_like(wf) if want_grad else None          # the dgrad's weight image
    _call(lib, m.pack_weight, wt.data_ptr(), wf.data_ptr(), _ptr(wd), cout, cin, k, s)
    x2 = src[op.src2] if op.src2 is not None else None
    _call(lib, m.conv_fwd_head if op.head else m.conv_fwd, src[op.src].data_ptr(), _ptr(x2), wf.data_ptr(), _ptr(bias), z.data_ptr(),
          b_, h, w, cin, op.cin_up, cout, k, st, int(op.src == "x"), s)
    run.shape[op.out] = (b_, ho, wo, cout)
    return z, dict(wd=wd, geo=(b_, h, w, cin, cout, k, st))


def _bn_act(lib, s, m, op, z, res, sv):
    """The BatchNorm statistics of z (.train(): the batch's, and the running ones move) and y = leaky(bn(z)) [+ res] -> y."""
    bn, dev = op.bn, z.device
    P, cout = z.numel() // z.shape[-1], z.shape[-1]
    mean = torch.empty(cout, device=dev, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    g, bt = _f32(bn.weight, "bn.weight of " + op.out), _f32(bn.bias, "bn.bias of " + op.out)
    if bn.training:
        rm, rv = _f32(bn.running_mean, "running_mean"), _f32(bn.running_var, "running_var")
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
        mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
        rm_new, rv_new = torch.empty_like(rm), torch.empty_like(rv)
        nb = entry(lib, m.channel_ws)(P, cout)
        ws = _ws(nb, dev)
        _call(lib, m.bn_stats, z.data_ptr(), P, cout, float(bn.eps), float(mom), rm.data_ptr(), rv.data_ptr(), rm_new.data_ptr(),
              rv_new.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), nb, s, what="yv3_train_bn_stats")
        with torch.no_grad():          # (copy_ moves the buffers' _version: the inference engine re-packs)
            bn.running_mean.copy_(rm_new)
            bn.running_var.copy_(rv_new)
    else:
        _call(lib, "yv3_train_bn_eval_stats", bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(bn.eps),
              mean.data_ptr(), invstd.data_ptr(), cout, s)
    y = torch.empty_like(z)
    _call(lib, m.bn_act_fwd, z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), g.data_ptr(), bt.data_ptr(), _ptr(res), y.data_ptr(),
          P, cout, s, what="yv3_train_bn_act_fwd")
    sv.update(mean=mean, invstd=invstd, gamma=g, beta=bt, train=int(bn.training))
    return y


def _prefix(run, m, bufs, bufs_b, logits):
    """Ops [0, run.prefix) on the inference engine (net.frozen_prefix): one forward of the net's prefix engine in the inference mode
    of PREFIX_MODE -- F32: the exact-fp32 plan; BF16 / BF16_ACT: the BF16 plan, which stores each activation once, in bf16, rounds
    no z, and runs layer 0 as the inference front (the training kernels round x, z's operands and, in BF16_ACT, zb and y) -- then
    the hand-over: every buffer a prefix op wrote and an op from run.prefix on reads is copied out of the plan, which the next
    forward overwrites, in the form its reader expects (F32: fp32 in bufs; BF16_ACT: the bf16 plane in bufs_b; BF16: that and, for a
    buffer read as a residual, its fp32 widening in bufs); a prefix head hands over its fp32 logits.  The prefix ops get their
    shape and need = False, and nothing else: no saved entry, no weight pack, no z."""
    n, ops = run.prefix, run.ops
    eng = run.net.prefix_engine(PREFIX_MODE[run.math], n)
    _, plan = eng.forward(run.x, logits=True)
    read = {b for op in ops[n:] for b in (op.src, op.src2, op.res) if b is not None}
    read_res = {op.res for op in ops[n:] if op.res is not None}
    for op, sp in zip(ops[:n], eng.specs):
        t = plan.layer_out[sp.name]
        run.shape[op.out] = (plan.B,) + tuple(t.shape[-3:])
        run.need[op.out] = False
        if op.head:
            bufs[op.out] = t.clone()
            logits[op.head_idx] = (bufs[op.out], t.shape[1], t.shape[2])
        elif op.out in read and m.bf16_operands:
            bufs_b[op.out] = t[0].view(torch.int16).clone()
            if m.cast_twins and op.out in read_res:                      # (fp32 y beside its bf16 copy: residuals are read from y)
                bufs[op.out] = _engine.from_planes(t, eng.dtype)
        elif op.out in read:
            bufs[op.out] = t.clone()


def net_forward(run, want_grad):
    """The training forward of the whole net up to the heads -> their logits [(fp32 NHWC tensor, h, w)] * 3; with want_grad the
    run keeps what the walk needs.  With run.prefix = n > 0 the inference engine runs ops [0, n) (_prefix)."""
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    m, x = MATH[run.math], run.x
    act = m.act_dtype == torch.int16           # activations in bf16 only: bufs holds x and the head logits, bufs_b the rest
    B, _, H, W = x.shape
    bufs = {"x": x}
    bufs_b = None                              # bf16 conv inputs (the inference front reads x itself)
    if m.bf16_operands:
        bufs_b = {} if run.prefix else {"x": _bf16(lib, s, x, x.numel(), 1, 1, "x")}
    src = bufs_b if m.bf16_operands else bufs  # what the convs read
    outs = bufs_b if act else bufs             # where a conv_bn_relu's output (a later op's residual) lives
    last = {}                                  # buffer -> index of the last op that reads it in the forward
    for i, op in enumerate(run.ops):
        last.update({b: i for b in (op.src, op.src2, op.res) if b is not None})
    keep = set()                               # act: the bf16 buffers the walk reads (the inputs of a wgrad)
    run.shape["x"] = (B, H, W, 3)
    run.need["x"] = run.input_grad
    logits = [None] * 3
    if run.prefix:
        _prefix(run, m, bufs, bufs_b, logits)
    for i, op in enumerate(run.ops[run.prefix:], run.prefix):
        c = op.conv
        params = [c.weight] + ([c.bias] if op.head else [op.bn.weight, op.bn.bias])
        run.need[op.out] = any(p.requires_grad for p in params) or run.need[op.src] or \
            (op.src2 is not None and run.need[op.src2]) or (op.res is not None and run.need[op.res])
        if want_grad and c.weight.requires_grad:
            keep.update(b for b in (op.src, op.src2) if b is not None)
        z, sv = _conv(lib, s, m, run, op, src, want_grad)
        if op.head:
            bufs[op.out] = z
            logits[op.head_idx] = (z, z.shape[1], z.shape[2])
        else:
            y = _bn_act(lib, s, m, op, z, outs[op.res] if op.res is not None else None, sv)
            outs[op.out] = y
            if m.cast_twins:                   # (every conv_bn_relu output is some conv's input)
                bufs_b[op.out] = _bf16(lib, s, y, y.numel() // y.shape[-1], y.shape[-1], y.shape[-1], op.out)
            if act and not (want_grad and run.need[op.out]):              # no walk will reach this op
                z = None
            sv["z"] = z
        run.saved[i] = sv
        if act:                                # a bf16 buffer lives until its last reader: a later op, or a wgrad of the walk
            for b in {op.src, op.src2, op.res} - {None}:
                if last[b] == i and b not in keep:
                    del bufs_b[b]
    if want_grad:
        run.bufs, run.bufs_b = bufs, bufs_b
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
    lib, s, dev, m = _ffi.lib(), _ffi.stream_ptr(), run.x.device, MATH[run.math]
    grads, pg = {}, {}         # buffer -> dL/dbuffer (NHWC fp32; "x": NCHW); id(param) -> dL/dparam

    def rec(i, **tensors):
        if run.trace is not None:
            run.trace.setdefault(i, {}).update({k: t.clone() for k, t in tensors.items() if t is not None})

    def give(i, buf, t):
        """Add t into the gradient of buf (takes ownership of t when buf has none yet)."""
        if buf in grads:
            rec(i, res_before=grads[buf])
            _call(lib, "yv3_train_add", t.data_ptr(), grads[buf].data_ptr(), t.numel(), s)
        else:
            grads[buf] = t
        rec(i, res_after=grads[buf])

    def dz_of(i, op, sv, dy):
        """dy -> the op's per-channel gradients (and its residual's) and (dz, dz as the convs read it: itself or a padded bf16 copy)."""
        _, ho, wo, cout = run.shape[op.out]
        P = sv["geo"][0] * ho * wo
        nb = entry(lib, m.channel_ws)(P, cout)
        ws = _ws(nb, dev)
        # bf16 activations: dz is born in bf16, in the padded rows the dgrad / wgrad kernels read
        dz = torch.empty(P * m.pad(cout), device=dev, dtype=torch.int16) if m.act_dtype == torch.int16 else torch.empty_like(dy)
        if op.head:
            db = torch.empty(cout, device=dev, dtype=torch.float32)
            _call(lib, m.bias_bwd, dy.data_ptr(), _ptr(scale), dz.data_ptr(), db.data_ptr(), P, cout, ws.data_ptr(), nb, s,
                  what="yv3_train_bias_bwd")
            pg[id(op.conv.bias)] = db
            rec(i, dz=dz, dbias=db)
        else:
            dgam, dbet = torch.empty(cout, device=dev, dtype=torch.float32), torch.empty(cout, device=dev, dtype=torch.float32)
            _call(lib, m.bn_act_bwd, sv["z"].data_ptr(), dy.data_ptr(), sv["mean"].data_ptr(), sv["invstd"].data_ptr(),
                  sv["gamma"].data_ptr(), sv["beta"].data_ptr(), dz.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), P, cout, sv["train"],
                  ws.data_ptr(), nb, s, what="yv3_train_bn_act_bwd")
            pg[id(op.bn.weight)], pg[id(op.bn.bias)] = dgam, dbet
            rec(i, dz=dz, dgamma=dgam, dbeta=dbet)
            if op.res is not None and run.need[op.res]:
                give(i, op.res, dy)    # y = act(...) + res: dres = dy (dy is not read again)
        return dz, _bf16(lib, s, dz, P, cout, m.pad(cout), "dz of " + op.out) if m.cast_twins else dz

    def wgrad(i, op, sv, dz):
        b_, h, w, cin, cout, k, st = sv["geo"]
        dw = torch.empty_like(op.conv.weight, dtype=torch.float32, memory_format=torch.contiguous_format)
        nw = entry(lib, m.conv_wgrad_ws)(b_, h, w, cin, cout, k, st)
        wsw = _ws(nw, dev)
        src = run.bufs_b if m.bf16_operands else run.bufs            # what the convs read
        x2 = src[op.src2] if op.src2 is not None else None
        _call(lib, m.conv_wgrad, src[op.src].data_ptr(), _ptr(x2), dz.data_ptr(), dw.data_ptr(), b_, h, w, cin, op.cin_up, cout,
              k, st, int(op.src == "x"), wsw.data_ptr(), nw, s)
        pg[id(op.conv.weight)] = dw
        rec(i, dw=dw)

    def dgrad(i, op, sv, dz):
        """dz into the gradients of those inputs of the op that need one."""
        need_src, need_src2 = run.need[op.src], op.src2 is not None and run.need[op.src2]
        if not (need_src or need_src2):
            return
        b_, h, w, cin, cout, k, st = sv["geo"]
        if op.src == "x":                  # layer 0: dL/dx in the caller's NCHW layout, from the parameter itself
            dx = torch.empty((b_, cin, h, w), device=dev, dtype=torch.float32)
            wt = _f32(op.conv.weight, "weight of " + op.out)
            _call(lib, m.conv0_dgrad, dz.data_ptr(), wt.data_ptr(), dx.data_ptr(), b_, h, w, cout, s)
            grads["x"] = dx
            rec(i, dx_after=dx)
            return

        def conv_dgrad(dx, acc):
            _call(lib, m.conv_dgrad, dz.data_ptr(), sv["wd"].data_ptr(), dx.data_ptr(), b_, h, w, cin, cout, k, st, int(acc), s)

        if op.cin_up == 0:
            acc = op.src in grads
            dx = grads[op.src] if acc else torch.empty((b_, h, w, cin), device=dev, dtype=torch.float32)
            rec(i, dx_before=dx if acc else None)
            conv_dgrad(dx, acc)
            grads[op.src] = dx
            rec(i, dx_after=dx)
            return
        dcat = torch.empty((b_, h, w, cin), device=dev, dtype=torch.float32)
        conv_dgrad(dcat, False)
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
        _call(lib, "yv3_train_upcat_bwd", dcat.data_ptr(), _ptr(dlow), _ptr(dtail), b_, h, w, op.cin_up, ct, acc_low, acc_tail, s)
        rec(i, dlow_after=dlow, dtail_after=dtail)

    grads.update({op.out: dlogits[op.head_idx] for op in run.ops if op.head and dlogits[op.head_idx] is not None})
    for i in range(len(run.ops) - 1, -1, -1):
        op, sv = run.ops[i], run.saved.get(i)     # (none for an op of the frozen prefix: its output is never needed)
        dy = grads.pop(op.out, None)
        if dy is None or not run.need[op.out]:
            continue
        rec(i, dy=dy)
        dz, dzc = dz_of(i, op, sv, dy)          # (dz lives as long as its copy)
        if op.conv.weight.requires_grad:
            wgrad(i, op, sv, dzc)
        dgrad(i, op, sv, dzc)
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
