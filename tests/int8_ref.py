"""The I8 math mode's definition restated in numpy, bit for bit: what the int8 kernels, the quantise kernel and
engine.pack_conv's host-side weight quantisation must equal.  Nothing here imports the engine: the wiring of the 68 int8 layers is
derived from arch.conv_specs and the architecture's routes alone.

    activations  x ~ s_t * q, q int8 in [-127, 127], one fp32 scale per tensor
    weights      w' = w * s_in(ci) (fp32); sw[co] = max|w'[co]| / 127 (1 if 0); qw = clip(rint(w' / sw[co]), -127, 127)
    product      exact int32
    epilogue     t = fmaf((float)acc, m[co], b[co]), m = sw * alpha;  v = max(t, 0.1f * t);  v = fmaf((float)q_res, s_res, v) with a residual;
                 q = clip(rint(v * inv_s_out), -127, 127), inv_s_out = 1.0f / s_out
"""
import numpy as np

from yolo_v3_amd import arch

F32 = np.float32
I8_FIRST = 4          # convolutions 0-3 and the three heads are not int8


def fmaf(a, b, c):
    """fp32 fused multiply-add, exactly: the product in float64 (exact: 24 x 24 bits), the sum with TwoSum, rounded to odd in float64
    (53 >= 2 * 24 + 2 bits), then once to float32."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=F32), np.asarray(b, dtype=F32), np.asarray(c, dtype=F32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.copy().view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    away = (err > 0) == (s > 0)                    # the exact sum lies further from zero than s
    bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(F32)


def input_scales(cin, s_x, cin_up=0, s_route=None):
    """s_in(ci): constant, or behind an upsample + concat the upsampled tensor's scale for the first cin_up channels and the route's
    for the rest."""
    s = np.full(cin, F32(s_x), dtype=F32)
    if cin_up:
        s[cin_up:] = F32(s_route)
    return s


def quantize_weights(w, s_in):
    """(qw [O,C,k,k] fp32 integers, sw [O] fp32)."""
    w1 = (np.asarray(w, dtype=F32) * np.asarray(s_in, dtype=F32)[None, :, None, None]).astype(F32)
    amax = np.abs(w1).reshape(w1.shape[0], -1).max(axis=1)
    sw = np.where(amax > 0, amax / F32(127.0), F32(1.0)).astype(F32)
    qw = np.clip(np.rint((w1 / sw[:, None, None, None]).astype(F32)), -127.0, 127.0).astype(F32)
    return qw, sw


def quantize_act(x, s):
    """fp32 (or bf16 values held in fp32) -> int8: clip(rint(x * (1.0f / s)), -127, 127), NaN -> 0."""
    inv = F32(1.0) / F32(s)
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.clip(np.rint((x * inv).astype(F32)), -127.0, 127.0)
    return np.where(np.isnan(x), 0.0, r).astype(np.int8)


def gather_input(xq, x2q=None):
    """The layer's input [B,H,W,C] int8: xq, or nearest x2 of xq followed by x2q's channels."""
    if x2q is None:
        return xq
    up = xq.repeat(2, axis=1).repeat(2, axis=2)
    return np.concatenate((up, x2q), axis=3)


def conv_acc(xq, qw, stride=1):
    """Exact int32 convolution sums [B,Ho,Wo,O] of int8 NHWC input and integer OIHW weights, pad (k-1)/2.  (float64 matmul: every
    partial sum is an integer below 2^53.)"""
    B, H, W, C = xq.shape
    O, _, k, _ = qw.shape
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, C), dtype=np.float64)
    xp[:, pad:pad + H, pad:pad + W] = xq
    cols = np.concatenate([xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride] for kh in range(k) for kw in range(k)], axis=3)
    wm = np.asarray(qw, dtype=np.float64).transpose(0, 2, 3, 1).reshape(O, k * k * C)
    acc = cols.reshape(-1, k * k * C) @ wm.T
    assert np.abs(acc).max(initial=0) < 2.0 ** 31
    return acc.astype(np.int64).astype(np.int32).reshape(B, Ho, Wo, O)


def epilogue(acc, m, b, s_out, res_q=None, s_res=None):
    """int32 sums -> the quantised output as fp32 integers in [-127, 127]."""
    t = fmaf(acc.astype(F32), np.asarray(m, dtype=F32), np.asarray(b, dtype=F32))
    v = np.maximum(t, (F32(0.1) * t).astype(F32))
    if res_q is not None:
        v = fmaf(res_q.astype(F32), F32(s_res), v)
    inv = F32(1.0) / F32(s_out)
    return np.clip(np.rint((v * inv).astype(F32)), -127.0, 127.0).astype(F32)


def conv_layer(xq, w, s_in, alpha, beta, s_out, stride=1, x2q=None, res_q=None, s_res=None):
    """One int8 layer from its fp32 parameters: int8 NHWC out."""
    qw, sw = quantize_weights(w, s_in)
    m = (sw * np.asarray(alpha, dtype=F32)).astype(F32)
    acc = conv_acc(gather_input(xq, x2q), qw, stride)
    return epilogue(acc, m, beta, s_out, res_q, s_res).astype(np.int8)


def patch_index(pix, k, stride, H, W):
    """Where the k x k input window of each output pixel lies.  pix: integer [P, 3] rows (b, yo, xo).  Returns (b, yi, xi, inside), each
    [P, k, k]: the image, the input coordinates clamped into the H x W picture, and whether the tap lies inside it (pad (k-1)/2: taps
    outside read zero).  Plain index arithmetic, so that a test can gather the windows wherever the tensor lives."""
    pix = np.asarray(pix, dtype=np.int64).reshape(-1, 3)
    pad = (k - 1) // 2
    t = np.arange(k, dtype=np.int64)
    yi = (pix[:, 1] * stride - pad)[:, None, None] + t[None, :, None] + 0 * t[None, None, :]
    xi = (pix[:, 2] * stride - pad)[:, None, None] + t[None, None, :] + 0 * t[None, :, None]
    inside = (yi >= 0) & (yi < H) & (xi >= 0) & (xi < W)
    b = np.broadcast_to(pix[:, 0][:, None, None], yi.shape)
    return b, np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1), inside


def gather_patches(xq, pix, k, stride, x2q=None):
    """The input windows [P, k, k, C] int8 of output pixels `pix` from the layer's int8 NHWC input: xq, or (x2q given) nearest x2 of xq
    followed by x2q's channels -- read from the two sources directly, without building the concatenated tensor."""
    H, W = (x2q if x2q is not None else xq).shape[1:3]
    b, yi, xi, inside = patch_index(pix, k, stride, H, W)
    if x2q is None:
        p = xq[b, yi, xi]
    else:
        p = np.concatenate((xq[b, yi // 2, xi // 2], x2q[b, yi, xi]), axis=3)
    return (p * inside[..., None]).astype(np.int8)


def layer_at_pixels(patches, w, s_in, alpha, beta, s_out, res_q=None, s_res=None, qw_sw=None):
    """One int8 layer from its fp32 parameters on a set of output pixels: patches [P, k, k, C] int8 (gather_patches), res_q [P, O] int8 or
    None -> [P, O] fp32 integers in [-127, 127], what conv_layer gives at those pixels.  qw_sw: quantize_weights(w, s_in), when the
    caller keeps it."""
    qw, sw = qw_sw if qw_sw is not None else quantize_weights(w, s_in)
    O = qw.shape[0]
    m = (sw * np.asarray(alpha, dtype=F32)).astype(F32)
    P = patches.shape[0]
    wm = np.asarray(qw, dtype=np.float64).transpose(0, 2, 3, 1).reshape(O, -1)           # (kh, kw, ci), as the patches are laid out
    acc = patches.reshape(P, -1).astype(np.float64) @ wm.T
    assert np.abs(acc).max(initial=0) < 2.0 ** 31
    return epilogue(acc.astype(np.int64).astype(np.int32), m, beta, s_out, res_q, s_res)


def fold_bn(gamma, bias, mean, var, eps=1e-5):
    """alpha = gamma / sqrt(var + eps), beta = bias - mean * alpha, separate fp32 roundings."""
    a = (np.asarray(gamma, dtype=F32) / np.sqrt((np.asarray(var, dtype=F32) + F32(eps)).astype(F32)).astype(F32)).astype(F32)
    return a, (np.asarray(bias, dtype=F32) - (np.asarray(mean, dtype=F32) * a).astype(F32)).astype(F32)


def wiring(specs):
    """{conv index: (source, route or None, residual or None)} by the architecture: Darknet-53's stages (a stride-2 conv, then residual
    blocks x + conv2(conv1(x))), the routes after stages 2 and 3, three branches of six convs and a head, each later branch fed by a 1x1
    conv on the previous branch's fifth conv, upsampled and concatenated in front of a route."""
    g, i, cur, routes = {}, 1, 0, []
    for nblk in arch.BACKBONE_BLOCKS:
        g[i] = (cur, None, None); cur = i; i += 1
        for _ in range(nblk):
            g[i], g[i + 1] = (cur, None, None), (i, None, cur)
            cur = i + 1; i += 2
        routes.append(cur)
    x, route = cur, None
    for b in range(3):
        if b:
            g[i] = (fifth, None, None); x = i; i += 1
            route = routes[4 - b]                  # stage 3's output (26x26x512) for the second branch, stage 2's (52x52x256) for the third
        for j in range(7):
            g[i] = (x, route if j == 0 else None, None)
            x = i; i += 1
            if j == 4:
                fifth = x
    assert i == len(specs) == 75
    return g


def int8_layers(specs):
    return [i for i, sp in enumerate(specs) if i >= I8_FIRST and sp.bn]


def scale_names(specs):
    return [specs[I8_FIRST - 1].name] + [specs[i].name for i in int8_layers(specs)]


def run_layers(specs, params, scales, front_q):
    """All 68 int8 layers chained from the quantised front output.  params: {conv index: (w OIHW, alpha, beta)}; scales: {name: s}.
    Returns {conv index: int8 NHWC} (index I8_FIRST - 1: front_q)."""
    g, out = wiring(specs), {I8_FIRST - 1: front_q}
    for i in int8_layers(specs):
        src, route, res = g[i]
        sp = specs[i]
        cin_up = specs[src].cout if route is not None else 0
        s_in = input_scales(sp.cin, scales[specs[src].name], cin_up, scales[specs[route].name] if route is not None else None)
        w, alpha, beta = params[i]
        out[i] = conv_layer(out[src], w, s_in, alpha, beta, scales[sp.name], sp.stride, out[route] if route is not None else None,
                            out[res] if res is not None else None, scales[specs[res].name] if res is not None else None)
    return out
