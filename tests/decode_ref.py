"""The YOLO head decode (YoloLayer.forward(x, img_dim); csrc/decode.hip, reference yololayer.py:31-59,97-105) and its gradient,
restated in torch on the CPU.  float64 is the reference; the same functions in float32 give the yardstick behind the GPU tests' bar.

    logits [B, 3*(5+C), H, W], channel = anchor*(5+C) + attr   ->   out [B, H*W*3, 5+C], row = (y*W + x)*3 + anchor
    cx = (s(tx) + x) stride    cy = (s(ty) + y) stride    w = e^tw (aw / stride) stride    h = e^th (ah / stride) stride
    conf, classes = s(t)                                                                    (s = sigmoid)

`decode` is differentiable by torch autograd; `decode_grad` is the closed form the kernel yv3_decode_bwd_nchw computes:
dlogits = dout * (stride s(1-s) for tx, ty; the decoded w, h for tw, th; s(1-s) for the rest)."""
import torch


def _rows(lg):
    """[B, 3*A, H, W] -> [B, H, W, 3, A] (a view)."""
    B, ch, H, W = lg.shape
    return lg.reshape(B, 3, ch // 3, H, W).permute(0, 3, 4, 1, 2)


def _unrows(t):
    """[B, H, W, 3, A] -> [B, 3*A, H, W]."""
    B, H, W, _, A = t.shape
    return t.permute(0, 3, 4, 1, 2).reshape(B, 3 * A, H, W)


def _anchors(anchors, stride, like):
    return torch.as_tensor(anchors, dtype=like.dtype).reshape(3, 2) / stride


def decode(lg, anchors, stride):
    """anchors: the head's three (w, h) pairs in input pixels, flat or [3][2]; stride = img_dim / H."""
    B, ch, H, W = lg.shape
    t = _rows(lg)
    an = _anchors(anchors, stride, lg)
    gx = torch.arange(W, dtype=lg.dtype).view(1, 1, W, 1)
    gy = torch.arange(H, dtype=lg.dtype).view(1, H, 1, 1)
    cx = (torch.sigmoid(t[..., 0]) + gx) * stride
    cy = (torch.sigmoid(t[..., 1]) + gy) * stride
    w = torch.exp(t[..., 2]) * an[:, 0] * stride
    h = torch.exp(t[..., 3]) * an[:, 1] * stride
    out = torch.cat((torch.stack((cx, cy, w, h), -1), torch.sigmoid(t[..., 4:])), -1)
    return out.reshape(B, H * W * 3, ch // 3)


def decode_grad(lg, anchors, stride, dout):
    """-> (dL/dlogits [B, 3*A, H, W] for dout = dL/dout [B, H*W*3, A], S): S is the scale of each element's derivative, laid out as
    dlogits -- stride for tx and ty, the decoded w and h for tw and th, 1 for the rest (the GPU tests normalise errors by |dout| S)."""
    B, ch, H, W = lg.shape
    t = _rows(lg)
    an = _anchors(anchors, stride, lg)
    s = torch.sigmoid(t)
    d = s * (1 - s)
    S = torch.ones_like(t)
    S[..., 0:2] = stride
    S[..., 2] = torch.exp(t[..., 2]) * an[:, 0] * stride
    S[..., 3] = torch.exp(t[..., 3]) * an[:, 1] * stride
    d[..., 0:2] = d[..., 0:2] * stride
    d[..., 2:4] = S[..., 2:4]
    return _unrows(dout.reshape(B, H, W, 3, ch // 3) * d), _unrows(S)
