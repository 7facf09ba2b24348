"""Every head path above 80 classes (heads wider than 256 channels), on the GPU: the head convolution in every math mode along every forced
path, the fused and the stand-alone decode, the decode backward, the YOLO loss, the training kernels at the head, and whole networks at
C = 81 and 123.  The cases and the host's restatement of the operands are tests/test_wide_heads_host.py's, which also shows that each
float64 reference alone meets the bar used here; the harnesses are the existing files' (test_gpu_conv_matrix.Conv / _run_paths,
test_gpu_f16_conv.Conv, test_gpu_train_edges, test_gpu_input_grad.decode_error, the training files' check_against_ref).  No bar is new:
conv_ref.F32_BAR for fp32 logits, rtol 1e-6 / atol 1e-7 of test_gpu_kernels.py::test_decode_non_square_and_small_classes for decoded
values, BAR_FACTOR times torch's fp32 CPU error for the decode backward and the training steps, test_yolo_loss_host's assert_components /
assert_grad, helpers.TOL and the BF16 / F16 criteria of test_class_counts_between_38_and_69 and test_gpu_f16_e2e.py for whole networks.

Every output buffer is NaN-filled with a NaN canary behind it; every element written and the canary intact is asserted throughout."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle_cpu as oc
from yolo_v3_amd import YoloLayer, YoloNet, WeightManager, _ffi, arch, detect, synth
from tests import conv_ref as cr, decode_ref as D, f16_ref, yolo_loss_ref as R
from tests import test_gpu_conv_matrix as cm, test_gpu_f16_conv as f16c, test_gpu_f16_e2e as f16e, test_gpu_input_grad as gi
from tests import test_gpu_train as gt, test_gpu_train_bf16 as gtb, test_gpu_train_bf16_act as gta, test_gpu_train_bf16_act_step as gts
from tests import test_gpu_train_edges as te, test_gpu_train_local as gl, train_ref as T, train_ref_bf16 as TB, train_ref_bf16_act as TA
from tests import test_wide_heads_host as H
from tests.helpers import TOL, assert_close_rel, check_result_convention, detector_dets, rel_err
from tests.test_yolo_loss_host import assert_components, assert_grad

pytestmark = pytest.mark.gpu

F32, BF16, F32X3, F32H2, F16 = _ffi.F32, _ffi.BF16, _ffi.F32X3, _ffi.F32H2, _ffi.F16
DEV = "cuda:0"
NAN = cm.NAN
DECODE_RTOL, DECODE_ATOL = 1e-6, 1e-7                           # test_gpu_kernels.py::test_decode_non_square_and_small_classes


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    yield
    torch.cuda.synchronize()


def _lib():
    return _ffi.lib()


# ----------------------------------------------------------------------------- A. the head convolution, every mode, every path
def head_conv(mode, C, shape="13x13", cin=None):
    """The head of C classes as test_gpu_conv_matrix.Conv (F16: test_gpu_f16_conv.Conv): 1x1, alpha == NULL, fp32 output, linear, cout_pad
    as engine.pack_conv pads it -- and the operands are the ones the host file judged the bars on."""
    c0, B, Hh, W = H.HEAD_SHAPES[shape]
    cin = c0 if cin is None else cin
    cout, seed = H.cout_of(C), H.head_seed(C, shape)
    kw = dict(cin=cin, cout=cout, k=1, stride=1, B=B, H=Hh, W=W, alpha_none=True, out_f32=True, cout_pad=H.cout_pad_of(mode, cout), act=cr.ACT_LINEAR, seed=seed)
    conv = f16c.Conv(**kw) if mode == F16 else cm.Conv(mode, **kw)
    return conv


@pytest.mark.parametrize("mode", list(H.MODES), ids=list(H.MODES))
def test_host_operands_are_the_device_operands(mode):
    """The operands the host file judges the bars on (test_wide_heads_host.head_operands) are the values the device holds for this file's cases."""
    mode = H.MODES[mode]
    for C, shape in ((81, "13x13"), (81, "5x3")):
        conv = head_conv(mode, C, shape)
        cin, B, Hh, W = H.HEAD_SHAPES[shape]
        x, w, beta = H.head_operands(mode, cin, conv.cout, B, Hh, W, H.head_seed(C, shape))
        assert torch.equal(conv.x_ref, x) and torch.equal(conv.w_ref, w) and torch.equal(conv.beta_ref, beta) and conv.alpha_ref is None


def head_paths(mode, conv):
    """(paths, names that must equal the first bit for bit): the default choice and every forced tile code of the mode."""
    paths = [("default", 0, 0, None)]
    if mode == F32:
        paths += [cm.LANES] + ([("tune0=2", 0, 2, None)] if conv.cout_pad % 128 == 0 else [])
    else:
        paths += [("code %d" % c, cm._tile(c), 0, None) for c in (f16c.CODES if mode == F16 else cm.PLANE_CODES[mode])]
    bitwise = [p[0] for p in paths[1:]]
    ws = None
    if mode == F32H2:                            # (another summation order: bar only)
        ws = torch.zeros(_lib().yv3_conv_workspace_bytes(), dtype=torch.uint8, device="cuda")
        paths.append(("stream-K", 0, 0, ws))
    return paths, bitwise, ws


@pytest.mark.parametrize("mode", list(H.MODES), ids=list(H.MODES))
@pytest.mark.parametrize("C,shape", H.HEAD_CASES, ids=["C%d-%s" % c for c in H.HEAD_CASES])
def test_head_conv_every_path_vs_fp64(C, shape, mode):
    """cout = 258 .. 915 (3 to 8 channel tiles of 128 in the plane modes, 9 to 29 of 32 in exact fp32; the last real tile holds 2, 5, 32, 128,
    1 or 19 channels, whole tiles beyond cout write nothing), M = 338 (ragged last row tile) and M = 15 (less than one tile): the default and
    every forced path bit-equal, each within the bar of float64 on the rounded operands, every element written, canary intact, status 0."""
    mode = H.MODES[mode]
    conv = head_conv(mode, C, shape)
    paths, bitwise, ws = head_paths(mode, conv)
    print("wide head | C=%d cout=%d cout_pad=%d M=%d mode %d | yv3_conv2d_kernel: %s" % (C, conv.cout, conv.cout_pad, conv.M, mode, _ffi.conv2d_kernel(conv.desc(None))))
    cm._run_paths(conv, paths, bitwise, what="C=%d %s mode %d" % (C, shape, mode))
    if ws is not None:
        assert int(ws[-4 * 512:].view(torch.int32).abs().sum()) == 0          # every stream-K hand-over flag consumed


def _launch_tuned(conv, t0, t1):
    y = conv.new_y()
    d = conv.desc(y, 0, t0)
    d.tune[1] = t1
    n = _lib().yv3_conv2d_launches(ctypes.byref(d))
    line = _ffi.conv2d_kernel(d)
    _ffi.check(_lib().yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), "yv3_conv2d")
    return y, n, line


@pytest.mark.parametrize("C", [123, 59])
def test_head_conv_f32_gemm_equals_tiles_bitwise(C):
    """Exact fp32, cout = cout_pad = 384 (the 128 x 128 GEMM tile) and 192 (256 x 64): the persistent GEMM forced on every row (tune[0] = 14,
    tune[1] = 3), with the library's split (14, 0) and by its own rule (0, 0) against the direct tiles (tune[0] = 13: GEMM never) -- the tune
    codes of test_gemm_f32_equals_tiles_bitwise -- bit for bit, each within the fp32 bar of float64."""
    conv = head_conv(F32, C)
    assert conv.cout % 64 == 0 and conv.cout_pad == conv.cout
    ref = conv.ref()
    tiles, n, line = _launch_tuned(conv, _ffi.T0_GEMM_NEVER, 0)
    conv.check(tiles, ref, what="C=%d tiles" % C)
    assert n == 1 and "GEMM" not in line
    for t0, t1 in ((_ffi.T0_GEMM_ALWAYS, _ffi.T1_GEMM_ALL_ROWS), (_ffi.T0_GEMM_ALWAYS, 0), (0, 0)):
        y, n, line = _launch_tuned(conv, t0, t1)
        print("wide head | C=%d tune %d,%d | %d launches | %s" % (C, t0, t1, n, line))
        conv.check(y, ref, what="C=%d tune %d,%d" % (C, t0, t1))
        assert (t0 != _ffi.T0_GEMM_ALWAYS or line.startswith("GEMM_")) and n in (1, 2)
        assert torch.equal(y[:conv.y_elems()], tiles[:conv.y_elems()]), "tune %d,%d differs from the tiles" % (t0, t1)


def test_head_conv_f32_gemm_by_the_rule():
    """C = 123 in exact fp32 at the smallest batch of 13 x 13 pictures whose 128 x 128 tiles fill one round of this device (256 CUs: B = 65,
    M = 10985, 86 x 3 tiles): the library takes the persistent GEMM by its own rule (tests/golden/conv_select_wide_heads.json pins that choice
    on the host), here launched -- bit-equal to the direct tiles, within the fp32 bar of float64."""
    ncu = cm._num_cu()
    B = next(b for b in range(1, 513) if cm._cdiv(b * 169, 128) * 3 >= ncu)
    cout = H.cout_of(123)
    conv = cm.Conv(F32, 256, cout, 1, 1, B, 13, 13, alpha_none=True, out_f32=True, cout_pad=cout, act=cr.ACT_LINEAR, seed=H.head_seed(123, "13x13") + 1)
    ref = conv.ref()
    tiles, n, line = _launch_tuned(conv, _ffi.T0_GEMM_NEVER, 0)
    conv.check(tiles, ref, what="B=%d tiles" % B)
    y, n, line = _launch_tuned(conv, 0, 0)
    print("wide head | C=123 B=%d M=%d on %d CUs | %d launches | %s" % (B, conv.M, ncu, n, line))
    assert line.startswith("GEMM_128x128 nt=3 ") and n in (1, 2)
    conv.check(y, ref, what="B=%d by the rule" % B)
    assert torch.equal(y[:conv.y_elems()], tiles[:conv.y_elems()])


# ----------------------------------------------------------------------------- B. the fused decode
@pytest.mark.parametrize("mode", ["BF16", "F16", "F32H2", "F32X3"])
@pytest.mark.parametrize("C", [81, 82, 123, 166])
def test_fused_decode_at_wide_heads(C, mode):
    """test_f16_fused_decode_writes_exactly_its_rows' layout (dec_out inside a NaN tensor, 37 rows before, 11 after) at attrib = 86, 87, 128
    and 171: anchor boundaries inside the second .. fourth channel tile or exactly on tile edges.  Exactly this scale's rows are written; with
    y bound and with y == NULL they equal yv3_decode of the same descriptor's logits bit for bit; the logits meet F32_BAR; the decoded rows
    equal tests/decode_ref on those logits in float64."""
    mode = H.MODES[mode]
    attrs = 5 + C
    B, Hh, W, before, after = 2, 13, 13, 37, 11
    rows = Hh * W * 3
    ntot = before + rows + after
    conv = head_conv(mode, C, cin=128)
    lib = _lib()
    outs = []
    for bind_y in (True, False):
        dets = torch.full((B, ntot, attrs), NAN, device="cuda")
        y = conv.new_y()
        d = conv.desc(y if bind_y else None)
        d.dec_out = dets.data_ptr() + before * attrs * 4
        d.dec_out_batch_stride = ntot * attrs
        d.dec_stride = 32.0
        for i, a in enumerate(cm.ANCHORS):
            d.dec_anchors[i] = a
        _ffi.check(lib.yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), "yv3_conv2d (fused decode)")
        torch.cuda.synchronize()
        assert int(conv.flags.item()) == 0
        assert bool(torch.isnan(dets[:, :before]).all()) and bool(torch.isnan(dets[:, before + rows:]).all()), "wrote outside its rows"
        assert not bool(torch.isnan(dets[:, before:before + rows]).any()), "a row of the scale was not written"
        if bind_y:
            conv.check(y, conv.ref(), what="head logits C=%d mode %d" % (C, mode))
            logits = y
        else:
            assert bool(torch.isnan(y).all())
        outs.append(dets)
    sep = torch.full((B, ntot, attrs), NAN, device="cuda")
    an = (ctypes.c_float * 6)(*cm.ANCHORS)
    _ffi.check(lib.yv3_decode(logits.data_ptr(), 3 * attrs, an, 32.0, sep.data_ptr() + before * attrs * 4, ntot * attrs, B, Hh, W, C, _ffi.stream_ptr()), "yv3_decode")
    torch.cuda.synchronize()
    assert bool(torch.isnan(sep[:, :before]).all()) and bool(torch.isnan(sep[:, before + rows:]).all())
    assert torch.equal(outs[0][:, before:before + rows], sep[:, before:before + rows])
    assert torch.equal(outs[1][:, before:before + rows], sep[:, before:before + rows])
    lg = logits[:conv.M * conv.cout].view(B, Hh, W, conv.cout).permute(0, 3, 1, 2).cpu().double()
    want = D.decode(lg, list(cm.ANCHORS), 32.0)
    np.testing.assert_allclose(outs[0][:, before:before + rows].cpu().numpy(), want.numpy(), rtol=DECODE_RTOL, atol=DECODE_ATOL)


# ----------------------------------------------------------------------------- C. the stand-alone decode, forward and backward
HUGE = [float("inf"), float("-inf"), 1e38, -1e38, 3e38, -3e38, 89.0, -104.0, 100.0, -110.0, float("nan"), 0.0]      # test_decode_non_finite_and_huge_logits_like_the_reference


def _decode_logits(B, C, Hh, W):
    """The host file's logits; where the head has channels >= 256, every value of HUGE in each attribute kind there (C = 300: x, y, w, h, conf
    and classes of anchors 1 and 2; C = 81: the last two classes of anchor 2)."""
    lg, dout, anchors, stride = H.decode_inputs(B, C, Hh, W)
    ch, A = lg.shape[1], 5 + C
    hot = list(range(256, ch))
    if hot:
        chans = [c for c in hot if c % A < 5] + [c for c in hot if c % A >= 5][:7]
        for i, c in enumerate(chans):
            for s in range(min(B * Hh * W, len(HUGE))):
                b, p = divmod(s, Hh * W)
                lg[b, c, p // W, p % W] = HUGE[(s + 4 * i) % len(HUGE)]
        assert bool(torch.isinf(lg[:, 256:]).any()) and bool(torch.isnan(lg[:, 256:]).any())
    return lg, anchors, stride


def _check_decoded(out, lg, anchors, stride, what):
    """Against tests/decode_ref in float64 where that is finite in fp32 too; infinities and NaN where the same map in fp32 has them."""
    ref, ref32 = D.decode(lg.double(), anchors, stride), D.decode(lg, anchors, stride)
    assert torch.equal(torch.isnan(out), torch.isnan(ref32)) and torch.equal(torch.isinf(out), torch.isinf(ref32)), what
    assert torch.equal(out[torch.isinf(ref32)], ref32[torch.isinf(ref32)]), what
    fin = torch.isfinite(ref32)
    np.testing.assert_allclose(out[fin].numpy(), ref[fin].numpy(), rtol=DECODE_RTOL, atol=DECODE_ATOL, err_msg=what)


@pytest.mark.parametrize("B,C,Hh,W", H.DECODE_SHAPES)
def test_decode_forward_at_wide_heads(B, C, Hh, W):
    """yv3_decode (NHWC, ld_logits = ch + 5, the padding NaN) and yv3_decode_nchw: ch = 258 and 915 make the 256-thread channel loop take a
    second and a fourth trip, 76 x 76 = 5776 pixels make the forward's pixel groups (1024 blocks of 4) wrap.  Bit-equal to each other."""
    lg, anchors, stride = _decode_logits(B, C, Hh, W)
    ch, A, lib = lg.shape[1], 5 + C, _lib()
    n = B * Hh * W * 3 * A
    an = (ctypes.c_float * 6)(*anchors)
    nchw = lg.cuda()
    nhwc = torch.full((B, Hh, W, ch + 5), NAN, device="cuda")
    nhwc[..., :ch] = nchw.permute(0, 2, 3, 1)
    outs = []
    for name in ("nhwc", "nchw"):
        out = torch.full((n + cm.CANARY,), NAN, device="cuda")
        if name == "nhwc":
            _ffi.check(lib.yv3_decode(nhwc.data_ptr(), ch + 5, an, stride, out.data_ptr(), Hh * W * 3 * A, B, Hh, W, C, _ffi.stream_ptr()), "yv3_decode")
        else:
            _ffi.check(lib.yv3_decode_nchw(nchw.data_ptr(), an, stride, out.data_ptr(), Hh * W * 3 * A, B, Hh, W, C, _ffi.stream_ptr()), "yv3_decode_nchw")
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[n:]).all()), "%s wrote past the end" % name
        got = out[:n].view(B, Hh * W * 3, A).cpu()
        _check_decoded(got, lg, anchors, stride, "%s %s" % (name, (B, C, Hh, W)))
        outs.append(out[:n])
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("B,C,Hh,W", H.DECODE_SHAPES)
def test_decode_backward_at_wide_heads(B, C, Hh, W):
    """yv3_decode_bwd_nchw through YoloLayer autograd, as test_gpu_input_grad.py::test_decode_backward, with its criterion (e <= BAR_FACTOR
    * e32 against torch fp32 CPU autograd): the channel loop's second and fourth trip, and at 76 x 76 the 4096-block pixel loop's wrap."""
    lg, dout, anchors, stride = H.decode_inputs(B, C, Hh, W)
    pairs = [tuple(arch.DEFAULT_ANCHORS[i:i + 2]) for i in range(0, 18, 2)]
    img_dim = (stride * W, stride * Hh)
    layer = YoloLayer(pairs, [3, 4, 5], img_dim, C)
    ld = lg.to(DEV)
    with torch.no_grad():
        plain = layer(ld, img_dim)
    lreq = ld.clone().requires_grad_(True)
    out = layer(lreq, img_dim)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    _check_decoded(plain.cpu(), lg, anchors, stride, "YoloLayer %s" % ((B, C, Hh, W),))
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    assert lreq.grad is not None and lreq.grad.shape == lreq.shape and bool(torch.isfinite(lreq.grad).all())
    e, e32 = gi.decode_error(lreq.grad, lg, dout, anchors, stride)
    print("decode backward %s: normalised error %.3g, torch fp32 CPU %.3g" % ((B, C, Hh, W), e, e32))
    assert e32 > 0 and e <= gi.BAR_FACTOR * e32


# ----------------------------------------------------------------------------- D. the loss
def _run_loss(layer, x, img_dim, tg, channels_last):
    xt = torch.from_numpy(x).to(DEV)
    if channels_last:
        xt = xt.contiguous(memory_format=torch.channels_last)
    xt.requires_grad_(True)
    out = layer(xt, img_dim, torch.from_numpy(tg))
    out[0].backward()
    torch.cuda.synchronize()
    return out, xt.grad


@pytest.mark.parametrize("C,same_cell", [(C, False) for C in H.LOSS_CLASSES] + [(123, True)], ids=["C81", "C123", "C300", "C123-two-classes-on-a-cell"])
def test_loss_at_wide_heads(C, same_cell):
    """A = 5 + C = 86, 128, 305 attributes per anchor: the cooperative gradient loop's nch exceeds (or equals half of) the 256-thread workgroup
    in both index splits -- NCHW (cell-fastest) and channels_last (channel-fastest) logits, bit-equal -- against the float64 restatement on a
    draw whose decisions all clear the margins; one case with two rows of different classes (5 and 122) on one cell."""
    spec, x, tg, res = H.loss_case(C, same_cell)
    B, img_dim = spec["B"], spec["img_dim"]
    layer = YoloLayer(R.ANCHORS, spec["mask"], img_dim, C)
    out, grad = _run_loss(layer, x, img_dim, tg, False)
    out_cl, grad_cl = _run_loss(layer, x, img_dim, tg, True)
    assert len(out) == 10 and torch.equal(out[0].detach(), out_cl[0].detach()) and tuple(out[1:]) == tuple(out_cl[1:])
    assert grad.shape == grad_cl.shape and torch.equal(grad.contiguous(), grad_cl.contiguous())
    assert [out[8], out[9]] == [res["nCorrect"], res["nGT"]] and res["nGT"] > 0
    want = R.stats_tuple(res, B)
    assert_components([v * B for v in out[2:8]], res["sums"])
    assert_components(float(out[0].detach()), res["sums"].sum())
    assert_components(out[1], want[0])
    assert bool(torch.isfinite(grad).all())
    assert_grad(grad.cpu().numpy(), res["grad"])


# ----------------------------------------------------------------------------- E. the training kernels at the head
@pytest.mark.parametrize("math", ["f32", "bf16"])
@pytest.mark.parametrize("cout", H.TRAIN_COUTS)
def test_training_head_conv(cout, math):
    """test_gpu_train_edges.py::test_conv_edges' head layer (1x1, bias) at cout = 258, 261 (BF16: padded to 264), 288 and 915 (920): forward with
    and without bias, dgrad (overwrite, accumulate), wgrad, both bf16 weight images, against that file's float64 references and bars."""
    te.test_conv_edges(H.train_case(cout), math)


@pytest.mark.parametrize("C,ld", [(258, 264), (261, 264)])
def test_cast_padded_wide(C, ld):
    """yv3_train_to_bf16's padded form (rows of C fp32 -> rows of ld bf16) at the widths _round8 gives the heads: torch's cast, the padding zero."""
    lib, s = _lib(), _ffi.stream_ptr()
    P = 37
    a = torch.randn(P, C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(C)) * 7
    d = torch.full((P * ld + gtb.CANARY,), 0x1234, device=DEV, dtype=torch.int16)
    _ffi.check(lib.yv3_train_to_bf16(a.data_ptr(), d.data_ptr(), P, C, ld, s))
    torch.cuda.synchronize()
    assert bool((d[P * ld:] == 0x1234).all())
    dd = d[:P * ld].view(P, ld)
    assert torch.equal(dd[:, :C], a.to(torch.bfloat16).view(torch.int16)) and bool((dd[:, C:] == 0).all())


@pytest.mark.parametrize("P", [1, 338])
@pytest.mark.parametrize("C", [258, 915])
@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_bias_bwd_wide(form, C, P):
    """yv3_train_bias_bwd and its _bf16 form with more channels than the suite's 255 (test_gpu_train_edges.py::test_bias_bwd,
    test_gpu_train_bf16_act.py::test_bias_bwd_bf16_values: their references and bars)."""
    for scale in (None, -1.75):
        (te.test_bias_bwd if form == "f32" else gta.test_bias_bwd_bf16_values)(scale, C, P)


# ----------------------------------------------------------------------------- F. whole networks
SIZE, NB = 96, 2


@pytest.fixture(scope="module", params=[81, 123], ids=["C81", "C123"])
def wide_net(request):
    """(C, the network on the GPU, images, the fp32 oracle's head logits and detections, the bf16 oracle's detections) -- built once per C."""
    C = request.param
    stream = synth.weight_stream(num_class=C, seed=78)
    net = YoloNet((SIZE, SIZE), numClass=C).eval()
    assert WeightManager(net).load_stream(stream) == stream.size
    net = net.cuda()
    sd, _ = oc.state_dict_from_stream(stream, C)
    x = torch.from_numpy(synth.images(NB, SIZE, 9))
    with torch.no_grad():
        logits = oc.head_logits(sd, x)
        ref = torch.cat(oc.yolonet_forward(sd, x, num_class=C), 1)
        ref_bf16 = torch.cat(oc.yolonet_forward(sd, x, num_class=C, prec="bf16"), 1)
    assert ref.shape == (NB, 3 * 21 * (SIZE // 32) ** 2, 5 + C)
    return C, net, x, logits, ref, ref_bf16


def _print_head_kernels(net, mode, C):
    plan = net.engine(mode).plan(NB, SIZE, SIZE)
    specs = arch.conv_specs(C)
    lines = [(specs[plan.desc_spec[j]].name, line) for j, line in zip(range(plan.first_desc, plan.n_desc), plan.kernels()) if not specs[plan.desc_spec[j]].bn]
    assert len(lines) >= 3 and all(specs[plan.desc_spec[j]].cout == H.cout_of(C) for j in range(plan.first_desc, plan.n_desc) if not specs[plan.desc_spec[j]].bn)
    print("wide net | C=%d mode %d | head kernels: %s" % (C, mode, "; ".join("%s: %s" % l for l in lines)))


@pytest.mark.parametrize("mode", ["F32H2", "F32X3", "F32", "BF16", "F16"])
def test_network_forward_vs_oracle(wide_net, mode):
    """forward_cat against the oracle with the criteria of test_class_counts_between_38_and_69 (TOL in the fp32 modes, BF16's mean relative
    error against the bf16 oracle); F16 with test_gpu_f16_e2e.py's: each head's logits error against the fp32 oracle at most a quarter of
    BF16's, measured in the same test."""
    C, net, x, logits, ref, ref_bf16 = wide_net
    mode = H.MODES[mode]
    net.math_mode = mode
    try:
        with torch.no_grad():
            dets = net.forward_cat(x.cuda()).cpu()
        torch.cuda.synchronize()
        assert net.engine(mode).dtype == mode
        _print_head_kernels(net, mode, C)
    finally:
        net.math_mode = F32H2
    assert dets.shape == ref.shape and bool(torch.isfinite(dets).all())
    if mode == BF16:
        e = float(rel_err(dets, ref_bf16).mean())
        print("wide net | C=%d BF16: mean relative error vs the bf16 oracle %.3g (bound 4e-3)" % (C, e))
        assert e < 4e-3
    elif mode == F16:
        e16 = [f16_ref.rel_l2(a, b) for a, b in zip(f16e._gpu_logits(net, x, F16), logits)]
        eb = [f16_ref.rel_l2(a, b) for a, b in zip(f16e._gpu_logits(net, x, BF16), logits)]
        print("wide net | C=%d logits vs the fp32 oracle, relative L2 per head | F16 %s | BF16 %s" % (C, " / ".join("%.3g" % v for v in e16), " / ".join("%.3g" % v for v in eb)))
        for a, b in zip(e16, eb):
            assert 0.0 < a <= b / 4, (e16, eb)
    else:
        e = assert_close_rel(dets, ref, TOL, "C=%d mode %d" % (C, mode))
        print("wide net | C=%d mode %d: max normalised error %.3g (TOL %g)" % (C, mode, e, TOL))


@pytest.mark.parametrize("is_eval", [False, True], ids=["nms", "eval"])
def test_network_detect_is_the_oracle_on_its_own_detections(wide_net, is_eval):
    """detect() in the default mode equals oracle_cpu.postprocess of the GPU's own forward_cat output bit for bit, NMS and eval mode: the staged
    candidate filter at 86 and 128 attributes per row.  Threshold 0.1: the oracle keeps 398 / 187 boxes (NMS) and 7516 / 2990 (eval) there."""
    C, net, x, _, _, _ = wide_net
    thr = 0.1
    net.math_mode = F32H2
    xd = x.cuda()
    with torch.no_grad():
        dets = net.forward_cat(xd).clone()
    got = detect(net, xd, C, thr, 0.4, is_eval=is_eval)
    torch.cuda.synchronize()
    assert torch.equal(detector_dets(net), dets)
    want = oc.postprocess(dets.cpu(), C, thr, 0.4, is_eval, True)
    check_result_convention(got, want)
    n = sum(len(b) for b in want)
    print("wide net | C=%d eval=%s: %d boxes at threshold %g" % (C, is_eval, n, thr))
    assert n >= 20
    for a, b in zip(got, want):
        assert tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu(), b)
        assert a.numel() == 0 or float(a[:, 6].max()) < C


@pytest.mark.parametrize("math", ["F32", "BF16", "BF16_ACT"])
def test_training_step_c81(math):
    """One train-mode step at C = 81 (heads 258 wide: 264 in the BF16 maths), 96 x 96, B = 2, against the float64 restatement of the math mode
    with the existing check_against_ref of its file; targets from that file's pick_target.  The images are the draw
    tests/test_wide_heads_host.py picks from the CPU references alone (STEP_IMAGES_SEED: the bar stands above what one LeakyReLU decision
    that fp32 cannot make may move).  On seed 31 the F32 step sits at 0.0346 against a bar of 0.0305 through one such decision, u = -1.04e-5
    in pre_det2.mlist.1, with every tensor downstream of it at 5e-5 and the heads' own gradients at 2e-6 .. 9e-6; the same images at C = 3,
    test_gpu_train.py's case, give 0.0293 under a bar of 0.27.  Every op of that seed-31 step is within its own bar:
    test_training_step_c81_every_op below."""
    C, hw = 81, (SIZE, SIZE)
    mcode = {"F32": _ffi.F32, "BF16": _ffi.BF16, "BF16_ACT": _ffi.BF16_ACT}[math]
    net = gl.make_net(hw, C, mcode).train()
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = gl.images(NB, hw, H.STEP_IMAGES_SEED)
    if math == "F32":
        logits, _, _ = T.forward(sd, x, True)
        tg = gt.pick_target(logits, SIZE, C, NB, 8, 77)
        loss = gt.gpu_step(net, x, tg)
        gt.check_against_ref(sd, net, loss, x, tg, C, True)
    elif math == "BF16":
        logits, _, _ = TB.forward(sd, x, True)
        tg = gtb.pick_target(logits, SIZE, C, NB, 8, 77)
        loss = gtb.gpu_step(net, x, tg)
        gtb.check_against_ref(sd, net, loss, x, tg, C, True)
    else:
        logits, _, _ = TA.forward(sd, x, True)
        tg = gtb.pick_target(logits, SIZE, C, NB, 8, 77)
        ref = TA.run(sd, x, tg, C, train=True)
        ref32 = TA.run(sd, x, tg, C, train=True, dtype=torch.float32)
        loss = gtb.gpu_step(net, x, tg)
        gts.check_against_ref(net, loss, ref, ref32, True)
    assert loss.requires_grad and int(net.feature.mlist[0].bn.num_batches_tracked) == 1
    for name in ("pre_det1", "pre_det2", "pre_det3"):
        head = getattr(net, name).mlist[6]
        assert tuple(head.weight.grad.shape)[0] == 258 and tuple(head.bias.grad.shape) == (258,) and float(head.weight.grad.abs().max()) > 0


@pytest.mark.parametrize("math", ["F32", "BF16"])
def test_training_step_c81_every_op(math):
    """The same step op by op (test_gpu_train_local.run_local_case: each of the 75 ops restated in float64 from the tensors the GPU fed it,
    the kernels' own bars, errors that do not compound; the traced and the untraced step bitwise equal) -- the head forward with bias, the
    loss gradient, bias_bwd, the head's wgrad and dgrad at cout = 258 (BF16: dz padded to 264) inside a real step."""
    gl.run_local_case((SIZE, SIZE), 81, NB, True, {"F32": _ffi.F32, "BF16": _ffi.BF16}[math], 31)
