"""The F16 math mode's kernels through the C-ABI (one fp16 plane on the BF16 tile set), against float64 on fp16-rounded operands with
the F16 bar (tests/conv_ref_f16.py: criteria A and B; fp32 head outputs conv_ref.F32_BAR): the shapes, forced tile codes, rule tiles,
fused-decode, batch-slice and error-contract cases of tests/test_gpu_conv_matrix.py's BF16 mode, yv3_conv0 with an F16 output, and the
saturation contract (status bit 0, +-65504 stored) on the conv2d paths, the fused front and the first residual block."""
import ctypes
import types

import pytest
import torch

from yolo_v3_amd import _ffi, engine
from tests import conv_ref as cr, conv_ref_f16 as cf
from tests import test_gpu_conv_matrix as cm
from tests.test_gpu_conv_matrix import (PLANE_CASES, BF16_RULE_CASES, BF16_RULE_KERNEL, BF16_RULE_LOOP, ERROR_CASES, ANCHORS, CANARY, NAN,
                                        SAT_CHANNEL, FP16_MAX)

pytestmark = pytest.mark.gpu

F16, F32 = _ffi.F16, _ffi.F32
CODES = (7, 8, 11, 13, 14, 15, 16)             # the forced tile codes of the one-plane kernels


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    yield
    torch.cuda.synchronize()


def _lib():
    return _ffi.lib()


def _f16(t):
    return t.half().float()


class Conv(cm.Conv):
    """test_gpu_conv_matrix.Conv in mode F16: the reference holds the fp16-rounded weights (packed unscaled, uniform in [-1, 1], so a
    few of them are fp16 subnormals), and check() applies the F16 bar."""

    def __init__(self, **kw):
        super().__init__(F16, **kw)
        self.w_ref = _f16(self.w_ref)

    def check(self, y, ref, pixels=None, what="", flag=0):
        torch.cuda.synchronize()
        n = self.y_elems()
        assert bool(torch.isnan(y[n:]).all()), "%s: wrote past the end of y" % what
        written = ~torch.isnan(y[:n])
        assert bool(written.all()), "%s: %d output elements not written" % (what, int((~written).sum()))
        assert int(self.flags.item()) == flag, "%s: status word %d" % (what, int(self.flags.item()))
        self.flags.zero_()
        got = self.read(y).double()
        if pixels is not None:
            got = got[pixels]
        if self.out_dtype == F32:
            e = cf.assert_f32_bar(got, ref, what)
            print("f16 bar | %s | fp32 out | max normalised error %.3g" % (what, e))
        else:
            r = cf.assert_f16(got, ref, self.mag(pixels), self.k * self.k * self.cin, what)
            print("f16 bar | %s | worst |d|/eps %.4g | share %.3g" % (what, r["worst"], r["share"]))
        return got


# ----------------------------------------------------------------------------- the layout helpers every reference below reads through
def test_split_and_merge_plane_f16_vs_torch():
    """yv3_split_plane_f16 == torch's fp32 -> fp16 (round to nearest even, subnormals kept) on values over 12 decades down into the
    subnormals, on ties and on the format's corners; beyond +-65504 (infinities included) it stores +-65504 where torch stores an
    infinity; NaN stays NaN.  yv3_merge_plane_f16 == torch's fp16 -> fp32, exactly.  engine.to_planes / from_planes are these two."""
    g = torch.Generator().manual_seed(5)
    v = (torch.rand(300000, generator=g) * 2 - 1) * 10.0 ** (torch.rand(300000, generator=g) * 12 - 9)        # 1e-9 .. 1e3
    corners = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -14), 2.0 ** -14 - 2.0 ** -25,
                            65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 7e4, -1e30, float("inf"), float("-inf"), float("nan")])
    x = torch.cat((v, corners)).cuda()
    assert int((v.abs() < 2.0 ** -14).sum()) > 50000
    n = x.numel()
    out = torch.full((n + CANARY,), NAN, dtype=torch.float16, device="cuda")
    _ffi.check(_lib().yv3_split_plane_f16(x.data_ptr(), out.data_ptr(), n, _ffi.stream_ptr()), "yv3_split_plane_f16")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all())
    want = x.clamp(-FP16_MAX, FP16_MAX).half()                      # (clamp keeps NaN)
    assert torch.equal(out[:n].view(torch.int16), want.view(torch.int16)), "%d elements differ" % int((out[:n].view(torch.int16) != want.view(torch.int16)).sum())
    finite = x.abs() <= FP16_MAX
    assert torch.equal(out[:n][finite].view(torch.int16), x[finite].half().view(torch.int16)) and bool(torch.isnan(out[n - 1]))
    assert out[n - 3].item() == FP16_MAX and out[n - 2].item() == -FP16_MAX
    back = torch.full((n + CANARY,), NAN, device="cuda")
    _ffi.check(_lib().yv3_merge_plane_f16(out.data_ptr(), back.data_ptr(), n, _ffi.stream_ptr()), "yv3_merge_plane_f16")
    torch.cuda.synchronize()
    assert bool(torch.isnan(back[n:]).all()) and torch.equal(back[:n - 1], out[:n - 1].float()) and bool(torch.isnan(back[n - 1]))
    t = x[:4096].view(2, 4, 8, 64)
    assert torch.equal(engine.to_planes(t, F16), t.half().unsqueeze(0)) and torch.equal(engine.from_planes(t.half().unsqueeze(0), F16), t.half().float())


# ----------------------------------------------------------------------------- the smallest shapes, default and every forced code
@pytest.mark.parametrize("name,kw", PLANE_CASES, ids=[c[0] for c in PLANE_CASES])
def test_f16_paths_vs_fp64(name, kw):
    """k3s1 / k3s2 / 1x1 with residual, cin_up 128 and 32, alpha == NULL, heads 18 / 75 / 255 with fp32 output, one image smaller than one
    tile: the default choice and every forced code (7, 8, 11, 13-16; a code the descriptor's features make the library decline gives the
    default's result) bit for bit equal to each other, each within the F16 bar of float64."""
    conv = Conv(seed=len(name) * 7 + F16, **kw)
    paths = [("default", 0, 0, None)] + [("code %d" % c, cm._tile(c), 0, None) for c in CODES]
    bitwise = [p[0] for p in paths[1:]]
    if conv.k == 3 and conv.stride == 1:
        paths.append(("k3s1", _ffi.OPT_K3S1, 0, None))             # (the kw-tap-reuse kernel: another summation order, bar only)
    cm._run_paths(conv, paths, bitwise, what="%s mode F16" % name)


# ----------------------------------------------------------------------------- the tiles the rules pick on large launches
@pytest.mark.parametrize("name,tile,kw", BF16_RULE_CASES, ids=[c[0] for c in BF16_RULE_CASES])
def test_f16_rule_tiles_vs_fp64_sampled(name, tile, kw):
    """The one-plane tiles that only large launches reach, each at the smallest batch at which the selection rule picks it on this
    device: yv3_conv2d_kernel names the tile for the F16 descriptor, the result meets the F16 bar on conv_ref.sample_rows and equals forced
    code 7 bit for bit."""
    ncu = cm._num_cu()
    cout_pad = kw.get("cout_pad", kw["cout"])
    Ho, Wo = cr.out_hw(kw["H"], kw["W"], kw["k"], 1)
    rule = lambda b: cm._bf16_tile_rule(b * Ho * Wo, cout_pad, kw["k"] == 3, kw.get("out_f32", False), ncu)
    B = next((b for b in range(1, 513) if rule(b)[0] == tile), None)
    assert B is not None, "%s: no batch up to 512 makes the rule pick the %s tile on %d CUs" % (name, tile, ncu)
    conv = Conv(B=B, seed=300 + len(name), **kw)
    line = _ffi.conv2d_kernel(conv.desc(None))
    print("f16 rule | %s | %d CUs | B = %d | yv3_conv2d_kernel: %s" % (name, ncu, B, line))
    assert line.split()[0] == BF16_RULE_KERNEL[tile] and line.split()[2] == BF16_RULE_LOOP[tile], (name, tile, line)
    rows = cr.sample_rows(conv.B, conv.Ho, conv.Wo, seed=5)
    cm._run_paths(conv, [("default", 0, 0, None), ("code 7", cm._tile(7), 0, None)], ["code 7"], pixels=rows, what=name)


# ----------------------------------------------------------------------------- yv3_conv0 with one fp16 plane out
@pytest.mark.parametrize("B,H,W", [(2, 40, 56), (1, 9, 131), (3, 64, 32), (1, 33, 260)])
def test_first_layer_f16_out_vs_fp64(B, H, W):
    """The matrix-core first layer with ONE fp16 plane out, on shapes with row / column tails and partial 128-column workgroup tiles:
    image and weights stay fp32, only the output is rounded -- the F16 bar with K = 27; status word 0."""
    g = torch.Generator().manual_seed(B * 1000 + H + W)
    x = torch.rand(B, 3, H, W, generator=g)
    w0, a0, b0 = cm._rand((32, 3, 3, 3), g, -0.3, 0.3), cm._rand((32,), g, 0.5, 1.5), cm._rand((32,), g, -0.2, 0.2)
    n = B * H * W * 32
    y = torch.full((n + CANARY,), NAN, dtype=torch.float16, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    dev = [t.cuda().contiguous() for t in (x, w0.permute(1, 2, 3, 0), a0, b0)]
    _ffi.check(_lib().yv3_conv0(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), y.data_ptr(), B, H, W, F16,
                                flags.data_ptr(), _ffi.stream_ptr()), "yv3_conv0")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[n:]).all()) and not bool(torch.isnan(y[:n]).any()) and int(flags.item()) == 0
    xh = x.permute(0, 2, 3, 1).contiguous()
    ref, mag = cr.conv_desc_ref(xh, w0, b0, a0), cr.conv_desc_mag(xh, w0, b0, a0)
    r = cf.assert_f16(y[:n].view(-1, 32).cpu().double(), ref, mag, 27, "yv3_conv0 F16 out %s" % ((B, H, W),))
    print("f16 bar | yv3_conv0 %s | worst |d|/eps %.4g | share %.3g" % ((B, H, W), r["worst"], r["share"]))


# ----------------------------------------------------------------------------- saturation
def _check_sat(conv, y, ref, mag, K, clipped, what):
    """`clipped`: bool [M, cout], the elements whose reference exceeds 65504 -- stored exactly as +65504, bit 0 set iff any; everything
    else within the F16 bar."""
    flag = 1 if bool(clipped.any()) else 0
    torch.cuda.synchronize()
    n = conv.y_elems()
    assert bool(torch.isnan(y[n:]).all()) and not bool(torch.isnan(y[:n]).any()), what
    assert int(conv.flags.item()) == flag, "%s: status word %d, expected %d" % (what, int(conv.flags.item()), flag)
    conv.flags.zero_()
    got = conv.read(y).double()
    assert bool((got[clipped] == FP16_MAX).all()), "%s: clipped values %s" % (what, got[clipped].unique()[:8].tolist())
    keep = ~clipped.any(1)                                # (whole rows: f16_report takes [rows, cout])
    if flag:
        keep_cols = ~clipped.any(0)
        cf.assert_f16(got[:, keep_cols], ref[:, keep_cols], mag[:, keep_cols], K, what)
    else:
        assert bool(keep.all())
        cf.assert_f16(got, ref, mag, K, what)


@pytest.mark.parametrize("case", ["a: just under", "b: one channel over", "c: one element under -65504"])
def test_f16_saturation_flag_every_conv2d_path(case):
    """F16 stores |value| > 65504 as +-65504 and ORs bit 0 into *flags (the engine's fall-back to BF16 hangs on it), on the default
    choice, every forced code and k3s1: (a) a channel peaking just under the limit keeps the bit clear, (b) a channel pushed over by
    beta = 7e4 sets it and stores exactly +65504 there, (c) ONE element (last M tile, last real channel) pushed under -65504 through its
    residual sets it and stores exactly -65504."""
    conv = Conv(cin=64, cout=512, k=3, stride=1, B=3, H=26, W=26, res=case.startswith("c"), seed=77)
    beta = conv.beta_ref.clone()
    if case.startswith("a"):
        beta[SAT_CHANNEL] = 64900.0
    elif case.startswith("b"):
        beta[SAT_CHANNEL] = 7.0e4
    else:
        beta[conv.cout - 1] = -100.0                                   # this channel's outputs are negative everywhere (leaky: x 0.1)
        r = conv.res_ref.clone().view(-1, conv.cout)
        r[conv.M - 1, conv.cout - 1] = -FP16_MAX
        conv.set_residual(r.view(conv.B, conv.Ho, conv.Wo, conv.cout))
    conv.set_beta(beta)
    ref, mag = conv.ref(), conv.mag()
    clipped = ref.abs() > FP16_MAX
    if case.startswith("a"):
        assert not bool(clipped.any()) and float(ref.max()) > 64800
    elif case.startswith("b"):
        assert bool(clipped[:, SAT_CHANNEL].all()) and int(clipped.sum()) == conv.M
    else:
        assert int(clipped.sum()) == 1 and bool(clipped[conv.M - 1, conv.cout - 1]) and float(ref[conv.M - 1, conv.cout - 1]) < 0
    paths = [("default", 0)] + [("code %d" % c, cm._tile(c)) for c in CODES] + [("k3s1", _ffi.OPT_K3S1)]
    for name, options in paths:
        y = conv.launch(options)
        torch.cuda.synchronize()
        got = conv.read(y).double()
        assert bool((got[clipped] == FP16_MAX * torch.sign(ref[clipped])).all()), "%s, %s: clipped values" % (case, name)
        want = 1 if bool(clipped.any()) else 0
        assert int(conv.flags.item()) == want, "%s, %s: status word %d" % (case, name, int(conv.flags.item()))
        conv.flags.zero_()
        cols = ~clipped.any(0)
        cf.assert_f16(got[:, cols], ref[:, cols], mag[:, cols], 9 * conv.cin, "%s, %s" % (case, name))
        n = conv.y_elems()
        assert bool(torch.isnan(y[n:]).all()) and not bool(torch.isnan(y[:n]).any())


def _pack(w, cout, k):
    p = torch.empty(cout * k * k * w.shape[1], device="cuda", dtype=torch.float16)
    _ffi.check(_lib().yv3_pack_conv_weight(w.cuda().data_ptr(), p.data_ptr(), cout, w.shape[1], k, cout, F16, _ffi.stream_ptr()), "yv3_pack_conv_weight")
    return p


@pytest.mark.parametrize("over", [False, True], ids=["just under", "one channel over"])
def test_f16_saturation_flag_conv_front(over):
    """yv3_conv_front_f16: beta1 of one channel just under 65504 keeps bit 0 clear, beta1 = 7e4 sets it and stores exactly +65504 in
    that channel; everything else within the F16 bar of the second layer's float64 reference on the first layer's own fp16 output
    (yv3_conv0 with an F16 output: the fused kernel computes that layer identically)."""
    B, H, W = 1, 64, 64
    g = torch.Generator().manual_seed(11)
    x = torch.rand(B, 3, H, W, generator=g)
    w0, a0, b0 = cm._rand((32, 3, 3, 3), g, -0.3, 0.3), cm._rand((32,), g, 0.5, 1.5), cm._rand((32,), g, -0.2, 0.2)
    w1, a1, b1 = cm._rand((64, 32, 3, 3), g), cm._rand((64,), g, 0.5, 1.5) / 288 ** 0.5, cm._rand((64,), g, -0.2, 0.2)
    b1[SAT_CHANNEL] = 7.0e4 if over else 64900.0
    w1p = _pack(w1, 64, 3)
    w0t = w0.permute(1, 2, 3, 0).contiguous().cuda()
    dev = [t.cuda() for t in (x, a0, b0, a1, b1)]
    n = B * (H // 2) * (W // 2) * 64
    y = torch.full((n + CANARY,), NAN, dtype=torch.float16, device="cuda")
    mid = torch.empty(B, H, W, 32, dtype=torch.float16, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ffi.check(_lib().yv3_conv0(dev[0].data_ptr(), w0t.data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), mid.data_ptr(), B, H, W, F16,
                                flags.data_ptr(), _ffi.stream_ptr()), "yv3_conv0")
    _ffi.check(_lib().yv3_conv_front_f16(dev[0].data_ptr(), w0t.data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), w1p.data_ptr(),
                                         dev[3].data_ptr(), dev[4].data_ptr(), y.data_ptr(), B, H, W, flags.data_ptr(), _ffi.stream_ptr()),
               "yv3_conv_front_f16")
    midh, w1h = mid.float().cpu(), _f16(w1)
    ref, mag = cr.conv_desc_ref(midh, w1h, b1, a1, stride=2), cr.conv_desc_mag(midh, w1h, b1, a1, stride=2)
    conv = types.SimpleNamespace(y_elems=lambda: n, flags=flags, read=lambda t: t[:n].view(-1, 64).float().cpu())
    _check_sat(conv, y, ref, mag, 288, ref > FP16_MAX, "yv3_conv_front_f16 over=%s" % over)


@pytest.mark.parametrize("over", [False, True], ids=["just under", "one channel over"])
def test_f16_saturation_flag_res_block64(over):
    """yv3_res_block64_f16 (1x1 64->32, 3x3 32->64, residual): the same two cases through beta2, against the float64 reference of the 3x3
    layer on the 1x1 layer's own fp16 output (its yv3_conv2d launch in F16: the fused kernel computes it identically)."""
    B, H, W = 2, 32, 48
    g = torch.Generator().manual_seed(12)
    x = _f16(cm._rand((B, H, W, 64), g))
    w1, a1, b1 = cm._rand((32, 64, 1, 1), g), cm._rand((32,), g, 0.5, 1.5) / 8.0, cm._rand((32,), g, -0.2, 0.2)
    w2, a2, b2 = cm._rand((64, 32, 3, 3), g), cm._rand((64,), g, 0.5, 1.5) / 288 ** 0.5, cm._rand((64,), g, -0.2, 0.2)
    b2[SAT_CHANNEL] = 7.0e4 if over else 64900.0
    p1, p2 = _pack(w1, 32, 1), _pack(w2, 64, 3)
    xp = x.half().cuda()
    dev = [t.cuda() for t in (a1, b1, a2, b2)]
    n = B * H * W * 64
    y = torch.full((n + CANARY,), NAN, dtype=torch.float16, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    mid = torch.empty(B, H, W, 32, dtype=torch.float16, device="cuda")
    d = _ffi.ConvDesc()
    d.x, d.w, d.alpha, d.beta, d.y = xp.data_ptr(), p1.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), mid.data_ptr()
    d.B, d.H, d.W, d.cin, d.cout, d.cout_pad, d.k, d.stride, d.act = B, H, W, 64, 32, 32, 1, 1, cr.ACT_LEAKY
    d.dtype = d.out_dtype = F16
    d.flags = flags.data_ptr()
    _ffi.check(_lib().yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), "yv3_conv2d 1x1")
    _ffi.check(_lib().yv3_res_block64_f16(xp.data_ptr(), p1.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), p2.data_ptr(),
                                          dev[2].data_ptr(), dev[3].data_ptr(), y.data_ptr(), B, H, W, flags.data_ptr(), _ffi.stream_ptr()),
               "yv3_res_block64_f16")
    midh, w2h = mid.float().cpu(), _f16(w2)
    ref, mag = cr.conv_desc_ref(midh, w2h, b2, a2, residual=x), cr.conv_desc_mag(midh, w2h, b2, a2, residual=x)
    conv = types.SimpleNamespace(y_elems=lambda: n, flags=flags, read=lambda t: t[:n].view(-1, 64).float().cpu())
    _check_sat(conv, y, ref, mag, 288, ref > FP16_MAX, "yv3_res_block64_f16 over=%s" % over)


# ----------------------------------------------------------------------------- fused decode, batch slices, errors
@pytest.mark.parametrize("num_class,cout_pad", [(20, 96), (80, 256)])
def test_f16_fused_decode_writes_exactly_its_rows(num_class, cout_pad):
    """dec_out in the middle of a NaN-filled [B, N_total, 5+C] tensor: exactly this scale's rows are written, they equal yv3_decode of the
    logits of the same descriptor bit for bit, y == NULL gives the same bits, and the logits meet the fp32 bar."""
    attrs = 5 + num_class
    B, H, W, before, after = 2, 13, 13, 37, 11
    rows = H * W * 3
    ntot = before + rows + after
    conv = Conv(cin=128, cout=3 * attrs, k=1, stride=1, B=B, H=H, W=W, alpha_none=True, out_f32=True, cout_pad=cout_pad, act=cr.ACT_LINEAR,
                seed=num_class + F16)
    lib = _lib()
    outs = []
    for bind_y in (True, False):
        dets = torch.full((B, ntot, attrs), NAN, device="cuda")
        y = conv.new_y()
        d = conv.desc(y if bind_y else None)
        d.dec_out = dets.data_ptr() + before * attrs * 4
        d.dec_out_batch_stride = ntot * attrs
        d.dec_stride = 32.0
        for i, a in enumerate(ANCHORS):
            d.dec_anchors[i] = a
        _ffi.check(lib.yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), "yv3_conv2d (fused decode)")
        torch.cuda.synchronize()
        assert int(conv.flags.item()) == 0
        assert bool(torch.isnan(dets[:, :before]).all()) and bool(torch.isnan(dets[:, before + rows:]).all()), "wrote outside its rows"
        assert not bool(torch.isnan(dets[:, before:before + rows]).any()), "a row of the scale was not written"
        if bind_y:
            conv.check(y, conv.ref(), what="head logits mode F16")
            logits = y
        else:
            assert bool(torch.isnan(y).all())
        outs.append(dets)
    sep = torch.full((B, ntot, attrs), NAN, device="cuda")
    an = (ctypes.c_float * 6)(*ANCHORS)
    _ffi.check(lib.yv3_decode(logits.data_ptr(), 3 * attrs, an, 32.0, sep.data_ptr() + before * attrs * 4, ntot * attrs, B, H, W,
                              num_class, _ffi.stream_ptr()), "yv3_decode")
    torch.cuda.synchronize()
    assert torch.equal(outs[0][:, before:before + rows], sep[:, before:before + rows])
    assert torch.equal(outs[1][:, before:before + rows], sep[:, before:before + rows])


def test_f16_batch_slice_equals_full_batch_bitwise():
    """A descriptor over images [b0, b0+Bs) of larger x / x2 / y / residual tensors, with cin_up and residual: rows outside the slice
    stay NaN, the slice equals the full-batch launch bit for bit."""
    B, b0, Bs = 6, 2, 3
    conv = Conv(cin=384, cout=256, k=1, stride=1, B=B, H=26, W=26, res=True, cin_up=128, seed=40 + F16)
    full = conv.launch()
    conv.check(full, conv.ref(), what="full batch mode F16")
    per_y = conv.Ho * conv.Wo * conv.cout
    per_x, per_x2 = 13 * 13 * 128, 26 * 26 * 256
    y = conv.new_y()
    d = conv.desc(y)
    es = y.element_size()
    d.x, d.x_plane_stride = conv.x.data_ptr() + b0 * per_x * es, B * per_x
    d.x2, d.x2_plane_stride = conv.x2.data_ptr() + b0 * per_x2 * es, B * per_x2
    d.y, d.y_plane_stride = y.data_ptr() + b0 * per_y * es, B * per_y
    d.residual = conv.res.data_ptr() + b0 * per_y * es
    d.B = Bs
    _ffi.check(_lib().yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), "yv3_conv2d (batch slice)")
    torch.cuda.synchronize()
    assert int(conv.flags.item()) == 0
    planes, fplanes = y[:B * per_y].view(B, per_y), full[:B * per_y].view(B, per_y)
    assert bool(torch.isnan(planes[:b0]).all()) and bool(torch.isnan(planes[b0 + Bs:]).all()) and bool(torch.isnan(y[B * per_y:]).all())
    assert torch.equal(planes[b0:b0 + Bs], fplanes[b0:b0 + Bs])


def test_f16_conv_error_contract():
    """For every invalid descriptor of the plane modes' error contract with dtype F16: yv3_conv2d, yv3_conv2d_form and yv3_conv2d_launches
    return the documented code and the NaN-filled y is untouched."""
    lib = _lib()
    B, H, W, cin, cout = 1, 4, 4, 64, 64
    big = 4 * 3 * B * H * W * 256
    bufs = {k: torch.zeros(big, dtype=torch.float16, device="cuda") for k in ("x", "x2", "w")}
    bufs["beta"] = torch.zeros(256, device="cuda")
    bufs["dec"] = torch.full((big,), NAN, device="cuda")
    y = torch.full((big,), NAN, dtype=torch.float16, device="cuda")
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    ptrs["other"] = _ffi.F32H2
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")

    def base():
        d = _ffi.ConvDesc()
        d.x, d.w, d.beta, d.y = ptrs["x"], ptrs["w"], ptrs["beta"], y.data_ptr()
        d.B, d.H, d.W, d.cin, d.cout, d.cout_pad, d.k, d.stride = B, H, W, cin, cout, cout, 1, 1
        d.act, d.dtype, d.out_dtype, d.flags = cr.ACT_LEAKY, F16, F16, flags.data_ptr()
        return d

    d = base()
    assert lib.yv3_conv2d_form(ctypes.byref(d)) == 0 and lib.yv3_conv2d_launches(ctypes.byref(d)) == 1
    failures = []
    for name, mutate, _, want in ERROR_CASES:
        if want is None:
            continue
        d = base()
        mutate(d, ptrs)
        got = (lib.yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), lib.yv3_conv2d_form(ctypes.byref(d)), lib.yv3_conv2d_launches(ctypes.byref(d)))
        ok = (got[0] == want and got[1] == 0 and got[2] == 1) if name.startswith("y NULL") else got == (want, want, want)
        if not ok:
            failures.append("%s: launch / form / launches = %s, expected %d" % (name, got, want))
    torch.cuda.synchronize()
    assert not failures, "\n".join(failures)
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(bufs["dec"]).all()) and int(flags.item()) == 0
