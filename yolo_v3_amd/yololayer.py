"""Drop-in surface of the reference's ``yololayer.py``.

``YoloLayer.forward(x, img_dim)`` turns head logits ``[B, 3*(5+C), H, W]`` (the reference's NCHW
layout, channel = anchor*(5+C)+attr, yololayer.py:42) into ``[B, H*W*3, 5+C]`` rows
``cx, cy, w, h, conf, cls...`` in input pixels (yololayer.py:45-59,98-104) with ONE fused HIP
kernel (``yv3_decode_nchw``); the reference does the box part on the CPU and crosses the
GPU<->CPU boundary twice (yololayer.py:58-59,98).  When ``x`` requires grad the decode is differentiable: the same
kernel forward, ``yv3_decode_bwd_nchw`` backward.  Inside ``YoloNet`` the NHWC variant
(``yv3_decode``) is used directly on the head conv's output, with no permute at all.

``YoloLayer.forward(x, img_dim, target)`` is the reference's training branch (yololayer.py:64-95,
107-172): it returns the same 10-tuple ``(loss, loss/nB, loss_x/nB, loss_y/nB, loss_w/nB, loss_h/nB,
loss_conf/nB, loss_cls/nB, nCorrect, nGT)``.  Targets, masks, the six loss terms and dL/dx are one
HIP call (``yv3_yolo_loss``, csrc/yololoss.hip) instead of the reference's CPU loop over images and
rows; the loss is differentiable with respect to ``x``.  Rows the reference cannot process raise
``Yv3Error`` (``code`` YV3_EINVAL), more than ``_ffi.YOLO_LOSS_MAX_ROWS`` valid rows in one image
``Yv3Error`` (YV3_ELIMIT).
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _ffi

HEAD_OUT_BYTES = 64        # per head: 6 fp64 sums, then int32 nCorrect, nGT, status (one device->host read for all heads)


def _error(msg, code):
    err = _ffi.Yv3Error(msg)
    err.code = code
    return err


def loss_target(target, B, device):
    """Targets ``[B, T, 5]`` (cls, cx, cy, w, h) from the CPU or the GPU as a contiguous fp32 tensor on `device`."""
    t = target if torch.is_tensor(target) else torch.as_tensor(np.asarray(target, dtype=np.float32))
    if t.dim() != 3 or t.shape[2] != 5:
        raise _error("target must be [B, T, 5] rows (cls, cx, cy, w, h), got %s" % (tuple(t.shape),), _ffi.ESHAPE)
    if t.shape[0] != B:
        raise _error("target holds %d images, the logits %d" % (t.shape[0], B), _ffi.ESHAPE)
    if t.shape[1] > 2 ** 31 - 1:
        raise _error("too many target rows", _ffi.ELIMIT)
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def launch_loss(x, strides, target, H, W, num_class, img_dim_h, anchors_all, mask, out, grad=None):
    """Enqueue ``yv3_yolo_loss`` for one head on the current stream.  x: fp32 logits on the GPU addressed by `strides`
    (batch, pixel, channel) in elements; out: ``HEAD_OUT_BYTES`` of device memory; grad: None or a tensor laid out like x."""
    lib = _ffi.lib()
    anchors = [float(v) for pair in anchors_all for v in pair]
    if len(anchors) != 18 or len(mask) != 3:
        raise _error("the loss needs the nine anchors (w, h) and a mask of three of them", _ffi.ESHAPE)
    d = _ffi.YoloLossDesc()
    d.logits, d.grad = x.data_ptr(), (grad.data_ptr() if grad is not None else None)
    d.stride_b, d.stride_p, d.stride_c = strides
    d.target = target.data_ptr() if target.numel() else None
    d.B, d.H, d.W, d.T, d.num_class = x.shape[0], H, W, target.shape[1], num_class
    d.img_dim_h = float(img_dim_h)
    for k in range(18):
        d.anchors[k] = anchors[k]
    for k in range(3):
        d.mask[k] = int(mask[k])
    base = out.data_ptr()
    d.sums, d.counts, d.status = base, base + 48, base + 56
    nbytes = lib.yv3_yolo_loss_workspace_bytes(d.B, H, W, d.T)
    if nbytes == 0:
        raise _error("loss shape out of range (B=%d, %dx%d, T=%d)" % (d.B, H, W, d.T), _ffi.ESHAPE)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    _ffi.check(lib.yv3_yolo_loss(ctypes.byref(d), ws.data_ptr(), nbytes, _ffi.stream_ptr()), "yv3_yolo_loss")


def head_results(host, k, nB):
    """Head k of the outputs read back (``HEAD_OUT_BYTES`` per head) -> (fp32 loss, the reference's 9 trailing values).
    Raises Yv3Error with the status code when the kernel rejected a row."""
    raw = host[k * HEAD_OUT_BYTES:(k + 1) * HEAD_OUT_BYTES]
    sums = np.frombuffer(raw[:48].tobytes(), dtype=np.float64)
    n_correct, n_gt, status = (int(v) for v in np.frombuffer(raw[48:60].tobytes(), dtype=np.int32))
    if status:
        msg = ("a target row the reference cannot process (class outside [0, numClass), a negative or NaN value, a cell outside "
               "the grid, or w*h > 2)" if status == _ffi.EINVAL else
               "more than %d valid target rows in one image" % _ffi.YOLO_LOSS_MAX_ROWS)
        raise _error("yv3_yolo_loss failed: %s (code %d)" % (msg, status), status)
    comps = [np.float32(v) for v in sums]                 # loss_x .. loss_cls as the reference's fp32 tensors
    loss = comps[0]
    for c in comps[1:]:
        loss = np.float32(loss + c)                       # loss_x + loss_y + loss_w + loss_h + loss_conf + loss_cls, fp32
    return loss, tuple([float(loss) / nB] + [float(c) / nB for c in comps] + [n_correct, n_gt])


def _loss_layout(x):
    """(fp32 tensor, (batch, pixel, channel) strides): x itself when its strides already address pixel y*W + x (NCHW
    contiguous, channels_last), else an NCHW copy."""
    if x.dtype == torch.float32 and (x.stride(2) == x.shape[3] * x.stride(3) or x.shape[2] == 1):
        return x, (x.stride(0), x.stride(3), x.stride(1))
    x = x.float().contiguous()
    return x, (x.stride(0), x.stride(3), x.stride(1))


class _YoloLossFn(torch.autograd.Function):
    """loss(x) with the kernel's dL/dx as its gradient; `box` receives the reference's nine trailing values."""

    @staticmethod
    def forward(ctx, x, layer, img_dim, target, want_grad, box):
        loss, rest, grad = layer._run_loss(x, img_dim, target, want_grad)
        box.append(rest)
        ctx.save_for_backward(grad if grad is not None else torch.empty(0))
        ctx.x_dtype = x.dtype
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        grad, = ctx.saved_tensors
        return (grad_output * grad).to(ctx.x_dtype), None, None, None, None, None


class _DecodeFn(torch.autograd.Function):
    """out = decode(x) (yv3_decode_nchw) with yv3_decode_bwd_nchw as its backward; x: contiguous fp32 logits."""

    @staticmethod
    def forward(ctx, x, layer, stride, anchors):
        ctx.save_for_backward(x)
        ctx.layer, ctx.stride, ctx.anchors = layer, stride, anchors
        return layer._decode(x, stride, anchors)

    @staticmethod
    def backward(ctx, dout):
        x, = ctx.saved_tensors
        nB, _, nH, nW = x.shape
        dout = dout.detach().to(device=x.device, dtype=torch.float32).contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _ffi.check(_ffi.lib().yv3_decode_bwd_nchw(x.data_ptr(), dout.data_ptr(), (ctypes.c_float * 6)(*ctx.anchors), ctx.stride,
                                                      dx.data_ptr(), nB, nH, nW, ctx.layer.numClass, _ffi.stream_ptr()),
                       "yv3_decode_bwd_nchw")
        return dx, None, None, None


class YoloLayer(nn.Module):
    def __init__(self, anchors_all, anchors_mask, img_dim, numClass):
        super().__init__()
        self.anchors_all = anchors_all          # list of (w, h) pairs, input pixels
        self.anchors_mask = anchors_mask
        self.img_dim = img_dim
        self.numClass = numClass
        self.bbox_attrib = 5 + numClass
        self.ignore_thres = 0.7                 # (fixed in the kernel, as in the reference)

    def _check_logits(self, x, what="head logits"):
        if not x.is_cuda:
            raise _ffi.GpuOnlyError("%s must live on the GPU: this package runs only on MI355X (HIP kernels), there is no CPU path"
                                    % what)
        if x.dim() != 4:
            raise _error("expected head logits [B, 3*(5+C), H, W], got %s" % (tuple(x.shape),), _ffi.ESHAPE)
        nB, ch, nH, nW = x.shape
        nA = len(self.anchors_mask)
        if nA != 3 or ch != nA * self.bbox_attrib:
            raise _error("expected %d channels (3 anchors x %d), got %d" % (3 * self.bbox_attrib, self.bbox_attrib, ch), _ffi.ESHAPE)
        return nB, nH, nW

    def _run_loss(self, x, img_dim, target, want_grad):
        """-> (0-d fp32 loss on x's device, the reference's 9 trailing values, dL/dx or None)."""
        nB, nH, nW = x.shape[0], x.shape[2], x.shape[3]
        xs, strides = _loss_layout(x.detach())
        with torch.cuda.device(x.device):
            t = loss_target(target, nB, x.device)
            grad = torch.empty_strided(xs.shape, xs.stride(), device=x.device, dtype=torch.float32) if want_grad else None
            out = torch.empty(HEAD_OUT_BYTES, device=x.device, dtype=torch.uint8)
            launch_loss(xs, strides, t, nH, nW, self.numClass, img_dim[1], self.anchors_all, self.anchors_mask, out, grad)
            loss, rest = head_results(out.cpu().numpy(), 0, nB)
            loss_t = torch.tensor(float(loss), dtype=torch.float32, device=x.device)
        return loss_t, rest, grad

    def forward(self, x, img_dim, target=None):
        if target is not None:
            self._check_logits(x)
            want_grad = bool(x.requires_grad and torch.is_grad_enabled())
            box = []
            loss = _YoloLossFn.apply(x, self, img_dim, target, want_grad, box)
            return (loss,) + box[0]
        _ffi.require_cuda(x, "head logits")
        nB, ch, nH, nW = x.shape
        nA = len(self.anchors_mask)
        if nA != 3 or ch != nA * self.bbox_attrib:
            raise _ffi.Yv3Error("expected %d channels (3 anchors x %d), got %d" % (3 * self.bbox_attrib, self.bbox_attrib, ch))
        stride = img_dim[1] / nH                                            # yololayer.py:36
        flat = []
        for m in self.anchors_mask:
            flat += [float(self.anchors_all[m][0]), float(self.anchors_all[m][1])]
        if x.requires_grad and torch.is_grad_enabled():                     # (x.float().contiguous() stays in autograd's graph)
            return _DecodeFn.apply(x.float().contiguous(), self, stride, flat)
        return self._decode(x.float().contiguous(), stride, flat)

    def _decode(self, x, stride, anchors):
        """yv3_decode_nchw on contiguous fp32 logits."""
        nB, _, nH, nW = x.shape
        out = torch.empty((nB, 3 * nH * nW, self.bbox_attrib), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _ffi.check(_ffi.lib().yv3_decode_nchw(x.data_ptr(), (ctypes.c_float * 6)(*anchors), stride, out.data_ptr(),
                                                  out.shape[1] * out.shape[2], nB, nH, nW, self.numClass,
                                                  _ffi.stream_ptr()), "yv3_decode_nchw")
        return out
