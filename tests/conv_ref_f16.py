"""The F16 kernels' bar: tests/conv_ref.py's BF16 bar (``bf16_report``) with fp16 in place of bfloat16.

A stored fp16 output `got`, the float64 result `ref` of the same descriptor on the same (fp16-held) operands: an fp16 x fp16 product is
exact in fp32 (11 + 11 bits), so got = f16(ref + fp32 summation and epilogue round-off), and the fp32 chain bound is conv_ref.bf16_eps,
unchanged:
    A  every element:  f16(ref - eps) <= got <= f16(ref + eps)
    B  the share of elements with got != f16(ref) is at most F16_SHARE_CAP = 2e-2.  A condition, not a measurement: fp16's spacing is 8
       times finer than bf16's against the same fp32 summation error, so a correct kernel flips about 8 times as often as under the bf16
       bar (cap 5e-3, measured 3.4e-4 on the GPU where the CPU stand-in gave 2.8e-4).  torch's fp32 convolution on the CPU gives
       7.4e-4 .. 4.5e-3 on the six shapes of tests/test_f16_host.py (the largest at K = 4608): the cap leaves about 4x; the mildest wrong
       epilogue there (LeakyReLU slope held in fp16) gives 0.18.
f16() is ONE rounding from float64 (ties to even), includes the subnormal range (quantum 2^-24) and saturates at +-65504, as the
kernels do.  fp32 outputs of an F16 conv (the heads) are not rounded at all: conv_ref.F32_BAR * max(1, |ref|)."""
import torch

from tests import conv_ref as cr

F16_SHARE_CAP = 2e-2
F16_MAX = 65504.0
F32_BAR = cr.F32_BAR


def round_f16_f64(t):
    """float64 -> the nearest fp16 value (ties to even), as float64: ONE rounding, where .float().half() would round twice.
    Normal range: frexp's |m| in [0.5, 1), so m * 2^11 has the format's 11 significant bits in front of the point.  Below 2^-14 the
    quantum stays 2^-24 (subnormals, kept); beyond +-65504 the value saturates (the kernels' fmed3), so 65520 and infinity give 65504."""
    t = t.double()
    m, e = torch.frexp(t)
    e = e.clamp(min=-13)                                  # |t| < 2^-14: the exponent of the smallest normal, i.e. quantum 2^-24
    q = torch.ldexp(torch.ones_like(t), e - 11)
    return (torch.round(t / q) * q).clamp(-F16_MAX, F16_MAX)


def f16_report(got, ref, mag, K):
    """Criteria A and B for stored fp16 values `got` [M, cout] against float64 `ref`, `mag` (same shape).  Returns a dict:
    worst = max |got - ref| / eps, share = fraction of got != f16(ref), outside = number of elements outside their interval,
    first = (row, channel) of the first of those or None, a_ok, b_ok."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape == mag.shape and got.dim() == 2 and bool(torch.isfinite(got).all())
    eps = cr.bf16_eps(K, mag.double())
    out = (got < round_f16_f64(ref - eps)) | (got > round_f16_f64(ref + eps))
    n_out = int(out.sum())
    first = divmod(int(out.reshape(-1).nonzero()[0]), got.shape[1]) if n_out else None
    share = float((got != round_f16_f64(ref)).double().mean())
    worst = float(((got - ref).abs() / eps.clamp(min=1e-300)).max())
    return dict(worst=worst, share=share, outside=n_out, first=first, a_ok=n_out == 0, b_ok=share <= F16_SHARE_CAP)


def assert_f16(got, ref, mag, K, what=""):
    """Assert A and B; the message carries the worst |got - ref| / eps, the share and the first element outside its interval."""
    r = f16_report(got, ref, mag, K)
    msg = "%s: worst |got - ref| / eps = %.4g (eps = (sqrt(%d) + 4) * 2^-24 * mag), share of got != f16(ref) = %.3g (cap %.1g), " \
          "%d elements outside [f16(ref - eps), f16(ref + eps)], the first at row/channel %s" % (
              what, r["worst"], K, r["share"], F16_SHARE_CAP, r["outside"], r["first"])
    assert r["a_ok"], "criterion A: " + msg
    assert r["b_ok"], "criterion B: " + msg
    return r


assert_f32_bar = cr.assert_f32_bar
