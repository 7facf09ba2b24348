"""Float64 restatement of what one ``yv3_conv_desc`` computes (include/yv3.h), for the kernel tests.

    y = act(conv(x_eff) * alpha + beta) (+ residual)

  * ``x_eff`` = cat(nearest_up2x(x), x2) along channels when ``cin_up > 0`` (darknet.py:161-162: the upsampled map first), else x;
  * ``alpha`` None means 1 (plain head conv, darknet.py:118);
  * pad = (k - 1) / 2 (darknet.py:34-35), stride 1 or 2;
  * ``act`` LEAKY is LeakyReLU(0.1) (darknet.py:41), LINEAR the identity;
  * the residual is added AFTER the activation (darknet.py:53).

Plain host torch, no GPU.  Tensors are NHWC as the kernels see them (already rounded to what the operand format represents: the
caller passes the values the planes hold); the weight is OIHW fp32.  Results are float64 rows [M, cout] (M = B*Ho*Wo, NHWC order),
or only the rows named in ``pixels`` -- computed by an explicit gather of their input patches, so that shapes of hundreds of 128-row
blocks stay cheap on the CPU.

The BF16 kernels' bar lives here too (``bf16_report`` / ``assert_bf16``): a stored bf16 output may differ from the float64 result of the
same operands only by the fp32 summation round-off and ONE round-to-nearest-even to bf16 (oracle/oracle_cpu.py, prec="bf16").
"""
import math

import torch
import torch.nn.functional as F

ACT_LINEAR, ACT_LEAKY = 0, 1
LEAKY_SLOPE = 0.1


def out_hw(H, W, k, stride):
    pad = (k - 1) // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _epilogue(acc, alpha, beta, act, residual_rows):
    v = acc * (alpha.double() if alpha is not None else 1.0) + beta.double()
    if act == ACT_LEAKY:
        v = torch.where(v > 0, v, LEAKY_SLOPE * v)
    elif act != ACT_LINEAR:
        raise ValueError("unknown activation %r" % (act,))
    if residual_rows is not None:
        v = v + residual_rows.double()
    return v


def _x_eff_nchw(x, x2, cin_up):
    xd = x.double().permute(0, 3, 1, 2)
    if not cin_up:
        return xd
    up = F.interpolate(xd, scale_factor=2, mode="nearest")
    return torch.cat((up, x2.double().permute(0, 3, 1, 2)), 1)


def _gather_rows(x, x2, cin_up, H, W, b, iy, ix):
    """x_eff[b, iy, ix, :] in float64 for index tensors b, iy, ix (zero outside the picture: the padding)."""
    valid = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    iyc, ixc = iy.clamp(0, H - 1), ix.clamp(0, W - 1)
    if cin_up:
        v = torch.cat((x[b, iyc // 2, ixc // 2].double(), x2[b, iyc, ixc].double()), 1)
    else:
        v = x[b, iyc, ixc].double()
    return v * valid.unsqueeze(1).double()


def conv_desc_ref(x, w, beta, alpha=None, residual=None, x2=None, cin_up=0, stride=1, act=ACT_LEAKY, pixels=None):
    """The descriptor's result in float64.

    x: NHWC [B, H, W, cin] -- or, with cin_up > 0, the low-resolution map [B, H/2, W/2, cin_up] and x2 = [B, H, W, cin - cin_up];
    w: OIHW [cout, cin, k, k]; beta [cout]; alpha [cout] or None; residual NHWC [B, Ho, Wo, cout] or None.
    pixels: None (every output row) or a 1-D tensor of flat output-row indices m = (b*Ho + oy)*Wo + ox.
    Returns float64 [M, cout] or [len(pixels), cout]."""
    cout, cin, k, k2 = w.shape
    assert k == k2 and k in (1, 3) and stride in (1, 2)
    if cin_up:
        assert x2 is not None and k == 1 and x.shape[3] == cin_up and x2.shape[3] == cin - cin_up
        B, H, W = x2.shape[0], x2.shape[1], x2.shape[2]
        assert x.shape[1] * 2 == H and x.shape[2] * 2 == W
    else:
        B, H, W = x.shape[0], x.shape[1], x.shape[2]
        assert x.shape[3] == cin
    Ho, Wo = out_hw(H, W, k, stride)
    pad = (k - 1) // 2
    if pixels is None:
        acc = F.conv2d(_x_eff_nchw(x, x2, cin_up), w.double(), None, stride, pad)          # [B, cout, Ho, Wo]
        acc = acc.permute(0, 2, 3, 1).reshape(B * Ho * Wo, cout)
        res = residual.reshape(B * Ho * Wo, cout) if residual is not None else None
        return _epilogue(acc, alpha, beta, act, res)
    m = torch.as_tensor(pixels, dtype=torch.long).reshape(-1)
    assert int(m.min()) >= 0 and int(m.max()) < B * Ho * Wo
    b, rem = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    wt = w.double().permute(0, 2, 3, 1)                                                       # [cout, kh, kw, cin]
    acc = torch.zeros(m.numel(), cout, dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            rows = _gather_rows(x, x2, cin_up, H, W, b, oy * stride + kh - pad, ox * stride + kw - pad)
            acc += rows @ wt[:, kh, kw, :].t()
    res = residual.reshape(B * Ho * Wo, cout)[m] if residual is not None else None
    return _epilogue(acc, alpha, beta, act, res)


def sample_rows(B, Ho, Wo, seed=0, n_random=2048, last=256):
    """The fixed sample of output rows for shapes too large for a full reference: every border row and column of image 0, the first
    and last pixel of every image, the last `last` rows of M (the last tile) and `n_random` seeded random rows.  Sorted, unique."""
    M = B * Ho * Wo
    oy, ox = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    border = ((oy == 0) | (oy == Ho - 1) | (ox == 0) | (ox == Wo - 1)).reshape(-1).nonzero().reshape(-1)
    firsts = torch.arange(B) * (Ho * Wo)
    parts = [border, firsts, firsts + Ho * Wo - 1, torch.arange(max(0, M - last), M),
             torch.randint(0, M, (n_random,), generator=torch.Generator().manual_seed(seed))]
    return torch.unique(torch.cat(parts))


# ----------------------------------------------------------------------------- the BF16 kernels' bar
# A stored bf16 output `got`, the float64 result `ref` of the same descriptor on the same (bf16-held) operands: a bf16 x bf16 product is
# exact in fp32, so got = bf16(ref + fp32 summation and epilogue round-off).  With the project's forward bound for an fp32-accumulated
# dot product (tests/test_gpu_configs.py::test_hostile_conv_level_all_fp32_modes, c = 4)
#       eps = (sqrt(K) + 4) * 2^-24 * mag,    K = k*k*cin,    mag = |alpha| * sum|w||x| + |beta| + |residual|
#   A  every element:  bf16(ref - eps) <= got <= bf16(ref + eps)        (bf16() is monotone: any value within eps of ref rounds into it)
#   B  the share of elements with got != bf16(ref) is at most BF16_SHARE_CAP -- a flip needs ref within eps of a rounding boundary,
#      and eps is ~1e-4 of the spacing of those; torch fp32 on the CPU gives 2e-5 .. 2.8e-4 (tests/test_conv_ref_host.py), the mildest faulty epilogue
#      there (LeakyReLU slope rounded to bf16) 9e-2.  A condition, not a measurement.
# fp32 outputs of a BF16 conv (the heads) are not rounded at all: F32_BAR * max(1, |ref|), the fp32 modes' bar.
BF16_SHARE_CAP = 5e-3
F32_BAR = 2e-5


def round_bf16_f64(t):
    """float64 -> the nearest bfloat16 value (ties to even), as float64: ONE rounding, where .float().bfloat16() would round twice.
    (frexp: |m| in [0.5, 1), so m * 2^8 has the format's 8 significant bits in front of the point; torch.round is half-to-even.)
    Normal range only, which is all these tests produce."""
    t = t.double()
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


def conv_desc_mag(x, w, beta, alpha=None, residual=None, x2=None, cin_up=0, stride=1, pixels=None):
    """|alpha| * sum|w||x| + |beta| + |residual|: conv_desc_ref on the absolute values of every operand, linear."""
    ab = lambda t: t.abs() if t is not None else None
    return conv_desc_ref(ab(x), ab(w), ab(beta), ab(alpha), ab(residual), ab(x2), cin_up, stride, ACT_LINEAR, pixels)


def bf16_eps(K, mag):
    return (math.sqrt(K) + 4.0) * 2.0 ** -24 * mag


def bf16_report(got, ref, mag, K):
    """Criteria A and B for stored bf16 values `got` [M, cout] against float64 `ref`, `mag` (same shape).  Returns a dict:
    worst = max |got - ref| / eps, share = fraction of got != bf16(ref), outside = number of elements outside their interval,
    first = (row, channel) of the first of those or None, a_ok, b_ok."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape == mag.shape and got.dim() == 2 and bool(torch.isfinite(got).all())
    eps = bf16_eps(K, mag.double())
    out = (got < round_bf16_f64(ref - eps)) | (got > round_bf16_f64(ref + eps))
    n_out = int(out.sum())
    first = divmod(int(out.reshape(-1).nonzero()[0]), got.shape[1]) if n_out else None
    share = float((got != round_bf16_f64(ref)).double().mean())
    worst = float(((got - ref).abs() / eps.clamp(min=1e-300)).max())
    return dict(worst=worst, share=share, outside=n_out, first=first, a_ok=n_out == 0, b_ok=share <= BF16_SHARE_CAP)


def assert_bf16(got, ref, mag, K, what=""):
    """Assert A and B; the message carries the worst |got - ref| / eps, the share and the first element outside its interval."""
    r = bf16_report(got, ref, mag, K)
    msg = "%s: worst |got - ref| / eps = %.4g (eps = (sqrt(%d) + 4) * 2^-24 * mag), share of got != bf16(ref) = %.3g (cap %.1g), " \
          "%d elements outside [bf16(ref - eps), bf16(ref + eps)], the first at row/channel %s" % (
              what, r["worst"], K, r["share"], BF16_SHARE_CAP, r["outside"], r["first"])
    assert r["a_ok"], "criterion A: " + msg
    assert r["b_ok"], "criterion B: " + msg
    return r


def assert_f32_bar(got, ref, what=""):
    """fp32 output of a BF16 conv: |got - ref| <= F32_BAR * max(1, |ref|)."""
    err = (got.double() - ref).abs() / ref.abs().clamp(min=1.0)
    assert float(err.max()) <= F32_BAR, "%s: max normalised error %.3g > %.1g at row/channel %s" % (
        what, float(err.max()), F32_BAR, divmod(int(err.argmax()), ref.shape[1]))
    return float(err.max())
