"""CPU pins of tests/conv_ref.py, the float64 restatement of yv3_conv_desc that tests/test_gpu_conv_matrix.py measures the kernels
against: it must equal the oracle's conv_bn_relu (darknet.py:27-44), the plain head conv (darknet.py:118), the residual add
(darknet.py:53) and UpsampleGroup's interpolate + cat (darknet.py:161-162), and its gathered `pixels` form must equal its full form.

The BF16 kernels' bar (conv_ref.bf16_report) is pinned here as well, without a GPU: torch's fp32 convolution with a correct epilogue
passes it on six shapes, and four subtly wrong epilogues, each of which passes the old 2e-2 * max(1, |ref|), fail it."""
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle_cpu as oc
from tests import conv_ref as cr


def _bn_state(cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    return {"c.conv.weight": (torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (3.0 / (cin * k * k)) ** 0.5,
            "c.bn.weight": torch.rand(cout, generator=g) * 0.6 + 0.6, "c.bn.bias": torch.rand(cout, generator=g) * 0.4 - 0.2,
            "c.bn.running_mean": torch.rand(cout, generator=g) * 0.4 - 0.2, "c.bn.running_var": torch.rand(cout, generator=g) * 0.7 + 0.7}


def _fold(sd):
    """alpha / beta of eval-mode BatchNorm2d (eps 1e-5), as yv3_fold_bn defines them -- in float64."""
    alpha = sd["c.bn.weight"].double() / torch.sqrt(sd["c.bn.running_var"].double() + 1e-5)
    return alpha, sd["c.bn.bias"].double() - sd["c.bn.running_mean"].double() * alpha


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _rows(t_nchw):
    return t_nchw.permute(0, 2, 3, 1).reshape(-1, t_nchw.shape[1])


@pytest.mark.parametrize("cin,cout,k,s,B,H,W", [(32, 64, 3, 1, 2, 7, 9), (32, 48, 3, 2, 3, 9, 7), (64, 32, 1, 1, 2, 5, 6),
                                                (32, 96, 3, 2, 1, 8, 10), (64, 24, 1, 1, 1, 1, 1)])
def test_reference_equals_conv_bn_leaky(cin, cout, k, s, B, H, W):
    sd = {key: v.double() for key, v in _bn_state(cin, cout, k, cin + cout + k).items()}
    x = torch.rand(B, cin, H, W, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2 - 1
    want = oc.cbr(sd, "c", x, stride=s)
    alpha, beta = _fold(sd)
    got = cr.conv_desc_ref(_nhwc(x), sd["c.conv.weight"], beta, alpha, stride=s, act=cr.ACT_LEAKY)
    assert got.dtype == torch.float64 and got.shape == (want.numel() // cout, cout)
    torch.testing.assert_close(got, _rows(want), rtol=1e-12, atol=1e-12)
    # ... and the residual goes on AFTER the activation (darknet.py:53): negative outputs of the sum survive
    r = torch.rand(want.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64) * 4 - 3
    got_r = cr.conv_desc_ref(_nhwc(x), sd["c.conv.weight"], beta, alpha, residual=_nhwc(r), stride=s)
    torch.testing.assert_close(got_r, _rows(want + r), rtol=1e-12, atol=1e-12)
    assert float(got_r.min()) < -1.0


def test_reference_plain_head_conv_alpha_none_linear():
    g = torch.Generator().manual_seed(5)
    w, b = torch.rand(75, 64, 1, 1, generator=g, dtype=torch.float64) - 0.5, torch.rand(75, generator=g, dtype=torch.float64) - 0.5
    x = torch.rand(2, 64, 5, 3, generator=g, dtype=torch.float64) - 0.5
    got = cr.conv_desc_ref(_nhwc(x), w, b, None, act=cr.ACT_LINEAR)
    torch.testing.assert_close(got, _rows(F.conv2d(x, w, b)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cin_up,ctail,B,h,w", [(32, 64, 2, 3, 5), (128, 32, 1, 4, 3), (64, 64, 3, 1, 1)])
def test_reference_upsample_concat(cin_up, ctail, B, h, w):
    """cin_up > 0: the input is cat(nearest_up2x(x), x2), the upsampled map first -- as F.interpolate(..., "nearest") + torch.cat."""
    g = torch.Generator().manual_seed(cin_up + ctail)
    up = torch.rand(B, cin_up, h, w, generator=g, dtype=torch.float64) - 0.5
    tail = torch.rand(B, ctail, 2 * h, 2 * w, generator=g, dtype=torch.float64) - 0.5
    wt = torch.rand(48, cin_up + ctail, 1, 1, generator=g, dtype=torch.float64) - 0.5
    alpha, beta = torch.rand(48, generator=g, dtype=torch.float64) + 0.5, torch.rand(48, generator=g, dtype=torch.float64) - 0.5
    cat = torch.cat((F.interpolate(up, scale_factor=2, mode="nearest"), tail), 1)
    want = F.leaky_relu(F.conv2d(cat, wt) * alpha.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1), 0.1)
    got = cr.conv_desc_ref(_nhwc(up), wt, beta, alpha, x2=_nhwc(tail), cin_up=cin_up)
    torch.testing.assert_close(got, _rows(want), rtol=1e-12, atol=1e-12)
    rows = cr.sample_rows(B, 2 * h, 2 * w, seed=1, n_random=7, last=5)
    torch.testing.assert_close(cr.conv_desc_ref(_nhwc(up), wt, beta, alpha, x2=_nhwc(tail), cin_up=cin_up, pixels=rows), got[rows],
                               rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("k,s,B,H,W,res", [(3, 1, 3, 11, 13, True), (3, 2, 2, 13, 11, False), (1, 1, 4, 9, 7, True), (3, 2, 1, 2, 3, True)])
def test_pixels_form_equals_full_form(k, s, B, H, W, res):
    g = torch.Generator().manual_seed(k * 100 + s * 10 + B)
    cin, cout = 32, 40
    x = torch.rand(B, H, W, cin, generator=g) * 2 - 1                       # float32 operands, as the kernels hold them
    w = torch.rand(cout, cin, k, k, generator=g) - 0.5
    alpha, beta = torch.rand(cout, generator=g) + 0.5, torch.rand(cout, generator=g) - 0.5
    Ho, Wo = cr.out_hw(H, W, k, s)
    r = torch.rand(B, Ho, Wo, cout, generator=g) - 0.5 if res else None
    full = cr.conv_desc_ref(x, w, beta, alpha, residual=r, stride=s)
    rows = cr.sample_rows(B, Ho, Wo, seed=2, n_random=50, last=16)
    part = cr.conv_desc_ref(x, w, beta, alpha, residual=r, stride=s, pixels=rows)
    torch.testing.assert_close(part, full[rows], rtol=1e-12, atol=1e-12)


def test_sample_rule():
    B, Ho, Wo = 37, 26, 27
    M = B * Ho * Wo
    rows = cr.sample_rows(B, Ho, Wo, seed=9)
    s = set(rows.tolist())
    assert rows.tolist() == sorted(s) and min(s) >= 0 and max(s) < M
    assert all(m in s for m in range(M - 256, M))                                            # the last tile
    assert all(b * Ho * Wo in s and (b + 1) * Ho * Wo - 1 in s for b in range(B))           # first / last pixel of every image
    assert all(oy * Wo + ox in s for oy in range(Ho) for ox in range(Wo) if oy in (0, Ho - 1) or ox in (0, Wo - 1))
    assert len(s) > 2000 and torch.equal(rows, cr.sample_rows(B, Ho, Wo, seed=9))


# ----------------------------------------------------------------------------- the BF16 bar: a correct stand-in passes, wrong epilogues fail
def test_round_bf16_f64_is_one_rounding():
    """Equal to torch's fp32 -> bf16 (oracle_cpu.round_bf16) on fp32 inputs, ties to even, and NOT double-rounded from float64."""
    g = torch.Generator().manual_seed(1)
    v = (torch.rand(200000, generator=g) * 2 - 1) * 10.0 ** (torch.rand(200000, generator=g) * 8 - 4)
    assert torch.equal(cr.round_bf16_f64(v.double()), oc.round_bf16(v).double())
    ties = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(2.0 + 2.0 ** -7), 0.0], dtype=torch.float64)
    assert cr.round_bf16_f64(ties).tolist() == [1.0, 1.0 + 2.0 ** -6, -2.0, 0.0]
    just_over = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)        # fp32 first would land on the tie, then on 1.0
    assert cr.round_bf16_f64(just_over).item() == 1.0 + 2.0 ** -7 and oc.round_bf16(just_over.float()).item() == 1.0


def _bf16_operands(cin, cout, k, s, B, H, W, res, alpha_none, seed):
    """The operand distributions of tests/test_gpu_conv_matrix.Conv in BF16 mode, as the planes hold them: x, w, residual rounded to
    bf16; alpha (fan-in scale) and beta fp32."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, lo, hi: torch.rand(shape, generator=g) * (hi - lo) + lo
    x = oc.round_bf16(u((B, H, W, cin), -1.0, 1.0))
    w = oc.round_bf16(u((cout, cin, k, k), -1.0, 1.0))
    alpha = None if alpha_none else u((cout,), 0.5, 1.5) / (cin * k * k) ** 0.5
    beta = u((cout,), -0.2, 0.2)
    Ho, Wo = cr.out_hw(H, W, k, s)
    r = oc.round_bf16(u((B, Ho, Wo, cout), -0.5, 0.5)) if res else None
    return x, w, alpha, beta, r


def _standin(x, w, alpha, beta, r, s, variant="correct"):
    """The BF16 conv as a kernel computes it, with torch's fp32 convolution standing in for the MFMA chain: fp32 accumulate, fp32
    epilogue, one rounding to bf16 -- or one of four wrong epilogues.  Returns fp32 [M, cout] holding bf16 values."""
    cout, k = w.shape[0], w.shape[2]
    acc = F.conv2d(x.permute(0, 3, 1, 2), w, None, s, (k - 1) // 2).permute(0, 2, 3, 1).reshape(-1, cout)
    b = oc.round_bf16(beta) if variant == "bf16 beta" else beta
    v = (acc * alpha if alpha is not None else acc) + b
    slope = float(oc.round_bf16(torch.tensor(0.1))) if variant == "bf16 slope" else 0.1
    v = torch.where(v > 0, v, torch.tensor(slope, dtype=torch.float32) * v)
    if variant == "double rounding":
        v = oc.round_bf16(v)
    if r is not None:
        v = v + r.reshape(-1, cout)
    if variant == "truncation":
        return (v.view(torch.int32) & -65536).view(torch.float32)
    return oc.round_bf16(v)


# cin, cout, k, stride, B, H, W, residual, alpha NULL      (K = 256 .. 4608)
BF16_SHAPES = [(256, 128, 1, 1, 2, 13, 13, True, False), (512, 256, 3, 1, 2, 13, 13, False, False), (128, 256, 3, 1, 3, 13, 11, True, False),
               (64, 128, 3, 2, 2, 27, 25, True, False), (64, 128, 3, 1, 2, 9, 11, True, True), (512, 256, 1, 1, 2, 7, 9, False, True)]


def _judge(case, seed, variant):
    cin, cout, k, s, B, H, W, res, alpha_none = case
    x, w, alpha, beta, r = _bf16_operands(cin, cout, k, s, B, H, W, res, alpha_none, seed)
    ref = cr.conv_desc_ref(x, w, beta, alpha, r, stride=s)
    mag = cr.conv_desc_mag(x, w, beta, alpha, r, stride=s)
    got = _standin(x, w, alpha, beta, r, s, variant)
    old = float(((got.double() - ref).abs() / ref.abs().clamp(min=1.0)).max())
    return got, ref, mag, k * k * cin, old


@pytest.mark.parametrize("case", BF16_SHAPES, ids=["%d-%d k%d s%d%s%s" % (c[0], c[1], c[2], c[3], " res" * c[7], " alphaNULL" * c[8])
                                                   for c in BF16_SHAPES])
def test_bf16_bar_passes_a_correct_fp32_accumulated_conv(case):
    got, ref, mag, K, old = _judge(case, 7, "correct")
    r = cr.assert_bf16(got, ref, mag, K, "torch fp32 stand-in %s" % (case,))
    assert old <= 2e-2                                    # (the share is 2e-5 .. 2.8e-4 here: a twentieth of the cap at most)


@pytest.mark.parametrize("variant", ["truncation", "double rounding", "bf16 beta", "bf16 slope"])
def test_bf16_bar_catches_wrong_epilogues_the_old_bar_passes(variant):
    """512->256 3x3 at 2 x 13 x 13 (K = 4608; with a residual for the double rounding, which needs one).  Each variant stays inside
    2e-2 * max(1, |ref|) and fails BOTH criteria.  B: the flips are 9 % (slope) to 50 % (truncation) of the elements, cap 0.5 %.
    A: eps is 4e-5 here (mag ~ sqrt(K) / 4), a twentieth of the bf16 spacing of an output near 0.2, so on the larger outputs almost
    every flip lands outside its interval; on outputs near zero, where eps spans several bf16 steps, only B can see them."""
    case = (512, 256, 3, 1, 2, 13, 13, variant == "double rounding", False)
    got, ref, mag, K, old = _judge(case, 11, variant)
    r = cr.bf16_report(got, ref, mag, K)
    assert old <= 2e-2, "the old bar was expected to pass this variant"
    assert not r["a_ok"] and r["first"] is not None and not r["b_ok"], r
    assert r["share"] >= 4 * cr.BF16_SHARE_CAP, r
    with pytest.raises(AssertionError, match="criterion A"):
        cr.assert_bf16(got, ref, mag, K, variant)
    ok = cr.bf16_report(_judge(case, 11, "correct")[0], ref, mag, K)
    assert ok["a_ok"] and ok["b_ok"], ok
