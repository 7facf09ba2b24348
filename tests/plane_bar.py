"""The bar of the fp32-class plane modes (F32H2: two fp16 planes hi + lo; F32X3: three bf16 planes) on REAL activations, and a CPU emulation
of an fp16-plane launch that the bar is checked against without a GPU (tests/test_plane_bar_host.py).  tests/test_gpu_plane_plan_local.py
holds every launch of the small plans to it.

The fixed kernel-test bar, 2e-5 * max(1, |ref|), is blind on real activations: there mag = |alpha| * sum|w||x| + |beta| + |residual| is 10 to
300 times |ref|, torch's own fp32 convolution reaches 2.8e-5 of max(1, |ref|) at the K = 4608 layers and an fp16 LeakyReLU slope stays far
below it.  So errors are counted in the unit of the fp32 dot-product bound (tests/test_gpu_configs.py::test_hostile_conv_level_all_fp32_modes):

    u = 2^-24 * mag      per output element, mag from conv_ref.conv_desc_mag on the same rows
                         (+ 2^-25 for an output stored as fp16 planes: half the spacing of fp16 subnormals, the resolution of `lo` below 2^-3)

  1  derived:   |got - ref| <= (sqrt(K) + 16) * u,  K = k*k*cin -- the project's bound for the split modes (c = 16: the operand representation,
     2^-23 relative each, and the dropped lo * lo product on top of the fp32 summation walk).  ref is float64 on the tensors the launch
     read, with the module's fp32 weights: the weight split belongs to the kernel's budget.
  2  relative to the reference's arithmetic: the launch's worst |got - ref| / u is at most DIRECT_X = 4 (direct forms) or WINO_X = 8
     (Winograd) times the worst |torch fp32 - ref| / u on the same rows of the same inputs (plan_ref.torch_f32_rows; never taken below one
     unit).  The multiples are tests/test_gpu_plan_local.py's.  The code under test never sets its bar.
  3  stored planes are a NEAREST split (full tensor): F32H2 |lo| <= half an fp16 ulp of hi; F32X3 each lower bf16 plane at most half an ulp
     of the plane above.  A truncating split fails this on about half the elements and is invisible to 1 and 2.
Head logits are fp32 outputs without a split: 1 and 2 without the 2^-25.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests import conv_ref as cr

U24 = 2.0 ** -24
FP16_PLANE_FLOOR = 2.0 ** -25
C_SPLIT = 16.0              # bar 1: (sqrt(K) + C_SPLIT) units
DIRECT_X, WINO_X = 4, 8     # bar 2: multiples of torch fp32's own error in units
OLD_BAR = 2e-5              # the fixed kernel-test bar, printed next to the new ones

Verdict = namedtuple("Verdict", "units torch bar1 bar2 old ok1 ok2 at")


def unit(mag, fp16_planes):
    """u per element (float64) from `mag`; fp16_planes: the output is stored as hi + lo fp16 planes."""
    return U24 * mag.double() + (FP16_PLANE_FLOOR if fp16_planes else 0.0)


def bar1_units(K):
    return math.sqrt(K) + C_SPLIT


def bar2_units(torch_units, wino=False):
    return (WINO_X if wino else DIRECT_X) * max(1.0, torch_units)


def judge(got, ref, mag, t32, K, wino=False, fp16_planes=True):
    """Bars 1 and 2 for one launch on its sampled rows.  got / t32: the launch's / torch fp32's rows [n, cout]; ref, mag float64 of the same
    shape.  units / torch: the worst error of either in u; old: the launch's worst error in the fixed 2e-5 bar; at: (row, channel) of the worst."""
    u = unit(mag, fp16_planes)
    e = (got.double() - ref).abs() / u
    worst, tu = float(e.max()), float(((t32.double() - ref).abs() / u).max())
    b1, b2 = bar1_units(K), bar2_units(tu, wino)
    old = float(((got.double() - ref).abs() / ref.abs().clamp(min=1.0)).max()) / OLD_BAR
    return Verdict(worst, tu, b1, b2, old, worst <= b1, worst <= b2, divmod(int(e.argmax()), ref.shape[1]))


# ----------------------------------------------------------------------------- check 3: the stored planes are a nearest split
_FORMAT = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}          # stored mantissa bits, exponent of the smallest normal


def half_ulp(t):
    """Half the spacing of the 16-bit format of `t` at each of its elements (float64; the subnormal spacing below the smallest normal).
    Built from the exponent field with integer arithmetic, so that it is EXACT on every device: |lo| equal to half an ulp is what a nearest
    split leaves at a tie (0.2 % of the elements of a bf16 plane), and a device power function that is not exact would call each of them a
    violation."""
    mant, emin = _FORMAT[t.dtype]
    field = ((t.contiguous().view(torch.int16).to(torch.int64) & 0x7FFF) >> mant).clamp(min=1)     # the biased exponent; subnormals: the smallest normal's
    e = field - (1 - emin) - mant - 1                                                               # half an ulp = 2^e
    return ((e + 1023) << 52).view(torch.float64)


def split_violations(planes):
    """planes [NP, ...] fp16 or bf16 (any device): the number of elements one of whose lower planes exceeds half an ulp of the plane above."""
    bad = torch.zeros(planes.shape[1:], dtype=torch.bool, device=planes.device)
    for i in range(1, planes.shape[0]):
        bad |= planes[i].double().abs() > half_ulp(planes[i - 1])
    return int(bad.sum())


# ----------------------------------------------------------------------------- CPU emulation of an fp16-plane launch
# Operands and outputs are hi + lo with torch.half (round to nearest even) splits, the three kept products w_hi x_hi + w_hi x_lo + w_lo x_hi
# run through fp32 F.conv2d, the epilogue (scale, shift, LeakyReLU, residual) in fp32 -- and the faults the fixed bar cannot see, each a switch.
FAULTS = ("drop_wlo_xhi", "drop_whi_xlo", "out_hi_only", "res_hi_only", "slope_fp16")


def split_h2(v):
    """fp32 -> (hi, lo): fp32 tensors holding the nearest fp16 split."""
    v = v.float()
    hi = v.half().float()
    return hi, (v - hi).half().float()


def trunc_split_h2(v):
    """The same with a hi that is TRUNCATED to fp16 (toward zero): what check 3 exists to catch."""
    v = v.float()
    normal = (v.view(torch.int32) & ~0x1FFF).view(torch.float32)                 # drop the 13 mantissa bits fp16 does not have
    tiny = torch.trunc(v * 2.0 ** 24) * 2.0 ** -24                                # below the smallest normal: multiples of 2^-24
    hi = torch.where(v.abs() >= 2.0 ** -14, normal, tiny).half().float()
    return hi, (v - hi).half().float()


def merge(pair):
    return pair[0] + pair[1] if isinstance(pair, tuple) else pair


def scaled_weight_h2(w):
    """engine.pack_conv's fp16-plane weights: every output channel scaled by its own power of two to max|w_row| in [1, 2) (not the
    3-channel first layer), split hi + lo; the inverse scale goes into the epilogue's alpha."""
    w = w.float()
    if w.shape[1] == 3:
        e = torch.zeros(w.shape[0])
    else:
        wmax = w.abs().amax(dim=(1, 2, 3))
        e = torch.where(wmax > 0, -torch.floor(torch.log2(wmax.clamp(min=1e-38))), torch.zeros_like(wmax)).clamp(-100.0, 100.0)
    hi, lo = split_h2(w * torch.exp2(e).view(-1, 1, 1, 1))
    return hi, lo, torch.exp2(-e)


def fault_applies(fault, node, p):
    return {"drop_wlo_xhi": node.spec.cin != 3, "drop_whi_xlo": node.spec.cin != 3, "out_hi_only": p.alpha is not None,
            "res_hi_only": node.residual is not None, "slope_fp16": p.act == cr.ACT_LEAKY}[fault]


def emulate_h2(node, p, x, x2=None, residual=None, faults=()):
    """One fp16-plane launch of `node` (plan_ref.Node, plan_ref.Params) on NHWC (hi, lo) pairs -> {None: the correct result, fault: the
    faulty one, ...}, each an NHWC (hi, lo) pair -- or, for a head (no BatchNorm), the fp32 logits."""
    def nchw(t):
        return t.permute(0, 3, 1, 2)

    def x_eff(i):
        if not node.cin_up:
            return nchw(x[i])
        return torch.cat((F.interpolate(nchw(x[i]), scale_factor=2, mode="nearest"), nchw(x2[i])), 1)

    wh, wl, unscale = scaled_weight_h2(p.w)
    s, pad = node.spec.stride, (node.spec.k - 1) // 2
    xh, xl = x_eff(0), x_eff(1)
    hh, hl, lh = F.conv2d(xh, wh, None, s, pad), F.conv2d(xl, wh, None, s, pad), F.conv2d(xh, wl, None, s, pad)
    alpha = ((p.alpha.float() if p.alpha is not None else torch.ones(p.w.shape[0])) * unscale).view(1, -1, 1, 1)
    beta = p.beta.float().view(1, -1, 1, 1)
    out = {}
    for fault in (None,) + tuple(faults):
        acc = hh + {None: hl + lh, "drop_wlo_xhi": hl, "drop_whi_xlo": lh}.get(fault, hl + lh)
        v = acc * alpha + beta
        if p.act == cr.ACT_LEAKY:
            slope = float(torch.tensor(cr.LEAKY_SLOPE).half()) if fault == "slope_fp16" else cr.LEAKY_SLOPE
            v = torch.where(v > 0, v, v * slope)
        if residual is not None:
            v = v + nchw(residual[0] if fault == "res_hi_only" else residual[0] + residual[1])
        v = v.permute(0, 2, 3, 1).contiguous()
        if p.alpha is None:
            out[fault] = v
        else:
            hi, lo = split_h2(v)
            out[fault] = (hi, torch.zeros_like(lo) if fault == "out_hi_only" else lo)
    return out


def mag_f32(node, p, x, x2=None, residual=None):
    """conv_desc_mag of EVERY output element in fp32 on the CPU, [M, cout]: the unit's scale (not a reference: 1e-3 of it would do) for the
    full-tensor comparison of two launch paths."""
    xin = x.float().abs().permute(0, 3, 1, 2)
    if node.cin_up:
        xin = torch.cat((F.interpolate(xin, scale_factor=2, mode="nearest"), x2.float().abs().permute(0, 3, 1, 2)), 1)
    y = F.conv2d(xin, p.w.abs(), None, node.spec.stride, (node.spec.k - 1) // 2)
    if p.alpha is not None:
        y = y * p.alpha.float().abs().view(1, -1, 1, 1)
    y = y + p.beta.float().abs().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.float().abs().permute(0, 3, 1, 2)
    return y.permute(0, 2, 3, 1).reshape(-1, node.spec.cout)
