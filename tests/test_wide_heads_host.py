"""Heads wider than 256 channels (more than 80 classes: cout = 3 * (5 + C) >= 258), on the host: the references and the bars the GPU file
tests/test_gpu_wide_heads.py relies on at the new widths, and the kernel selection of such heads.

  1  the oracle (oracle_cpu.yolonet_forward) at C = 81 and 123 against a plain conv2d + float64 decode of the same weight stream, and
     tests/decode_ref's decode / closed-form gradient at ch = 258 and 915 against torch autograd in float64;
  2  every kernel-level case of the GPU file: its float64 reference, rounded to the output type, passes the project's own bar with nothing
     excluded (conv_ref.F32_BAR, plane_bar bars 1 and 2, conv_ref / conv_ref_f16 criteria A and B with a share of 0, train_kernel_ref's
     CONV_BAR / BN_BAR), and the loss cases' decisions clear yolo_loss_ref.MARGIN;
  3  yv3_conv2d's choice for the head of every class count below in every math mode, against tests/golden/conv_select_wide_heads.json
     (tools/make_golden_conv_select.py --wide-heads): C = 123 in exact fp32 takes the persistent GEMM once its tiles fill a round of the
     device, C = 81 never.

The cases themselves (class counts, shapes, the operand draw of tests/test_gpu_conv_matrix.Conv restated without a device) are defined
here and imported by the GPU file."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle_cpu as oc
from yolo_v3_amd import _ffi, arch, synth
from tests import conv_ref as cr, conv_ref_f16 as cf, conv_select_grid as grid, decode_ref as D, plane_bar as pb
from tests import train_kernel_ref as K, yolo_loss_ref as R
from tests import test_gpu_train_edges as te
from tests.test_gpu_conv_matrix import _rand

F32, BF16, F32X3, F32H2, F16 = _ffi.F32, _ffi.BF16, _ffi.F32X3, _ffi.F32H2, _ffi.F16
MODES = {"F32H2": F32H2, "F32X3": F32X3, "BF16": BF16, "F16": F16, "F32": F32}

#  C    cout   why
#  81   258    first past 256; cout % 4 = 2; plane pad 384 (the third tile holds 2 real channels); F32 pad 288; BF16-train pad 264
#  82   261    cout % 4 = 1
#  91   288    cout % 32 = 0 (F32: cout_pad == cout), cout % 4 = 0 (no tail lane); plane pad 384
#  123  384    3 x 128 without a padded tile; attrib = 128: anchor boundaries on tile edges; GEMM-eligible in exact fp32
#  166  513    one real channel in the fifth tile; plane pad 640
#  300  915    plane pad 1024; the post-processing test's 300
CLASSES = (81, 82, 91, 123, 166, 300)
# (cin, B, H, W): M = 338 leaves a ragged last row tile; M = 15 is less than one tile
HEAD_SHAPES = {"13x13": (256, 2, 13, 13), "5x3": (128, 1, 5, 3)}
HEAD_CASES = [(C, "13x13") for C in CLASSES] + [(81, "5x3")]
DECODE_SHAPES = [(2, 81, 3, 5), (1, 300, 2, 2), (1, 1, 76, 76)]         # (B, C, H, W): channel loop wraps / wraps 3 times / 5776 pixels > 4096 blocks
TRAIN_COUTS = (258, 261, 288, 915)
LOSS_CLASSES = (81, 123, 300)


def cout_of(C):
    return 3 * (5 + C)


def cout_pad_of(mode, cout):
    """engine.pack_conv's padding: 32 channels, and whole 128-channel tiles in the plane modes above 128."""
    p = (cout + 31) // 32 * 32
    return (p + 127) // 128 * 128 if mode != F32 and p > 128 else p


def head_seed(C, shape):
    return 7000 + C + (500 if shape == "5x3" else 0)


def held(t, mode):
    """The fp32 values the operand format of `mode` holds for t (engine.to_planes -> from_planes, on the host)."""
    if mode == BF16:
        return t.bfloat16().float()
    if mode == F16:
        return t.half().float()
    if mode == F32H2:
        return pb.merge(pb.split_h2(t))
    return t.clone()                          # F32; F32X3: three bf16 planes hold all 24 bits of a value in [-1, 1] drawn as k * 2^-24


def head_operands(mode, cin, cout, B, H, W, seed):
    """(x_ref NHWC, w_ref OIHW, beta_ref) of test_gpu_conv_matrix.Conv / test_gpu_f16_conv.Conv for a plain head (k = 1, alpha == NULL, no
    residual): the same generator, the same order of draws, the rounding of the mode's operand format."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = held(_rand((B, H, W, cin), g), mode)
    w = _rand((cout, cin, 1, 1), g)
    w_ref = w.bfloat16().float() if mode == BF16 else w.half().float() if mode == F16 else w
    beta = _rand((cout,), g, -0.2, 0.2)
    return x, w_ref, beta


def loss_spec(C, same_cell=False):
    """The shape of yolo_loss_ref.CASES' m345_c80 at C classes; same_cell: two rows of different classes on one cell (the "quirks" rows)."""
    spec = dict(name="wide_c%d%s" % (C, "_same_cell" if same_cell else ""), seed=40 + C % 40 + (7 if same_cell else 0), B=2, C=C, mask=[3, 4, 5],
                img_dim=(128, 128), H=8, W=8, T=10, size=(0.1, 0.5))
    return spec


def loss_case(C, same_cell=False):
    """(spec, x, target, float64 result) of the first draw whose decisions all clear the margins (the search of the fixture's writer)."""
    spec = loss_spec(C, same_cell)
    for attempt in range(100):
        x, tg = R.make_case(spec, attempt)
        if same_cell:
            # rows 0 and 1 of image 0: the same cell and anchor (sizes 1 % apart, best anchor 3 at stride 16), another class each
            tg[0, 0] = [5, (3 + 0.35) / 8, (2 + 0.4) / 8, 0.22, 0.40]
            tg[0, 1] = [C - 1, (3 + 0.62) / 8, (2 + 0.55) / 8, 0.22 * 1.01, 0.40 * 0.99]
        res = R.yolo_loss(x, tg, R.ANCHORS, spec["mask"], spec["img_dim"][1], C)
        if R.margins_ok(res["margins"]) and res["nGT"] > 0:
            return spec, x, tg, res
    raise AssertionError("no draw of %s clears the margins" % spec["name"])


def train_case(cout):
    return ("head-%d-bias" % cout, 2, 13, 13, 256, cout, 1, 1, dict(bias=True))


# ----------------------------------------------------------------------------- 1. the references at the new widths
@pytest.mark.parametrize("C", [81, 123])
def test_oracle_heads_beyond_80_classes(C):
    """64 x 64, B = 1: each head's logits are conv2d(input of the head conv, its [3*(5+C), cin, 1, 1] slice of the stream) + bias -- here in
    float64 on the oracle's own activation -- and each scale's detections the float64 decode of those logits."""
    stream = synth.weight_stream(num_class=C)
    specs = arch.conv_specs(C)
    assert stream.size == arch.floats_in_stream(specs) and [s.cout for s in specs if not s.bn] == [cout_of(C)] * 3
    sd, used = oc.state_dict_from_stream(stream, C)
    x = torch.from_numpy(synth.images(1, 64, 5))
    taps = []
    with torch.no_grad():
        logits = oc.head_logits(sd, x, taps)
        dets = oc.yolonet_forward(sd, x, num_class=C)
    taps = dict(taps)
    for k, (pre, lg, det) in enumerate(zip(("pre_det1", "pre_det2", "pre_det3"), logits, dets)):
        h = 2 << k
        assert tuple(lg.shape) == (1, cout_of(C), h, h) and tuple(det.shape) == (1, 3 * h * h, 5 + C)
        w, b = sd[pre + ".mlist.6.weight"], sd[pre + ".mlist.6.bias"]
        assert tuple(w.shape) == (cout_of(C), taps[pre + ".mlist.5"].shape[1], 1, 1) and torch.equal(taps[pre + ".mlist.6"], lg)
        ref = F.conv2d(taps[pre + ".mlist.5"].double(), w.double(), b.double())
        cr.assert_f32_bar(K.rows(lg), K.rows(ref), "oracle %s logits C=%d" % (pre, C))
        anchors = [oc.DEFAULT_ANCHORS[2 * m + j] for m in ((6, 7, 8), (3, 4, 5), (0, 1, 2))[k] for j in (0, 1)]
        want = D.decode(lg.double(), anchors, 64.0 / h)
        np.testing.assert_allclose(det.numpy(), want.numpy(), rtol=1e-6, atol=1e-7)            # (test_decode_non_square_and_small_classes' tolerance)


@pytest.mark.parametrize("ch", [258, 915])
def test_decode_ref_gradient_is_autograd_at_wide_heads(ch):
    g = torch.Generator().manual_seed(ch)
    lg = (torch.rand(2, ch, 3, 5, generator=g, dtype=torch.float64) * 8 - 4).requires_grad_(True)
    dout = torch.randn(2, 3 * 5 * 3, ch // 3, generator=g, dtype=torch.float64)
    anchors, stride = [30.0, 61.0, 62.0, 45.0, 59.0, 119.0], 16.0
    out = D.decode(lg, anchors, stride)
    assert tuple(out.shape) == (2, 45, ch // 3)
    out.backward(dout)
    closed, S = D.decode_grad(lg.detach(), anchors, stride, dout)
    assert float(((closed - lg.grad).abs() / (D._unrows(dout.reshape(2, 3, 5, 3, -1)).abs() * S + 1e-300)).max()) <= 1e-14
    # the row / channel maps at this width: row (y*W + x)*3 + a, attribute j of anchor a is channel a*(ch/3) + j
    a, y, xx, j = 2, 1, 4, ch // 3 - 1
    assert float(out.detach()[1, (y * 5 + xx) * 3 + a, j]) == float(torch.sigmoid(lg.detach()[1, a * (ch // 3) + j, y, xx]))


# ----------------------------------------------------------------------------- 2. the bars at the new shapes
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
@pytest.mark.parametrize("C,shape", HEAD_CASES, ids=["C%d-%s" % c for c in HEAD_CASES])
def test_head_conv_reference_meets_its_bars(C, shape, mode):
    """The float64 logits of a head case, rounded to fp32 (the heads' output type): within conv_ref.F32_BAR and, counted in units of the fp32
    dot-product bound, within plane_bar's bars 1 and 2 against torch's own fp32 convolution.  Rounded to the mode's 16-bit type instead
    (what a plane output would store): criteria A and B with a share of exactly 0."""
    cin, B, H, W = HEAD_SHAPES[shape]
    x, w, beta = head_operands(MODES[mode], cin, cout_of(C), B, H, W, head_seed(C, shape))
    ref = cr.conv_desc_ref(x, w, beta, act=cr.ACT_LINEAR)
    mag = cr.conv_desc_mag(x, w, beta)
    assert tuple(ref.shape) == (B * H * W, cout_of(C))
    e = cr.assert_f32_bar(ref.float(), ref, "C=%d %s %s" % (C, shape, mode))
    t32 = F.conv2d(x.permute(0, 3, 1, 2), w, beta).permute(0, 2, 3, 1).reshape(ref.shape)
    v = pb.judge(ref.float(), ref, mag, t32, cin, fp16_planes=False)
    assert v.ok1 and v.ok2 and v.old <= 1.0, v
    cr.assert_f32_bar(t32, ref, "torch fp32")
    if MODES[mode] == BF16:
        r = cr.assert_bf16(cr.round_bf16_f64(ref), ref, mag, cin)
        assert r["share"] == 0.0 and r["outside"] == 0
    if MODES[mode] == F16:
        r = cf.assert_f16(cf.round_f16_f64(ref), ref, mag, cin)
        assert r["share"] == 0.0 and r["outside"] == 0 and cf.F16_SHARE_CAP == 2e-2
    print("C=%d %s %s: fp32-rounded reference %.3g of the fixed bar, %.3g units (bar 1 %.1f, bar 2 %.1f)" % (C, shape, mode, e / cr.F32_BAR, v.units, v.bar1, v.bar2))


@pytest.mark.parametrize("B,C,H,W", DECODE_SHAPES)
def test_decode_reference_meets_its_tolerance(B, C, H, W):
    lg, dout, anchors, stride = decode_inputs(B, C, H, W)
    ref = D.decode(lg.double(), anchors, stride)
    np.testing.assert_allclose(ref.float().numpy(), ref.numpy(), rtol=1e-6, atol=1e-7)
    gref, S = D.decode_grad(lg.double(), anchors, stride, dout.double())
    assert bool(torch.isfinite(gref).all()) and tuple(gref.shape) == tuple(lg.shape)


def decode_inputs(B, C, H, W):
    g = torch.Generator().manual_seed(100 * H + C)
    lg = torch.rand(B, cout_of(C), H, W, generator=g) * 8 - 4
    dout = torch.randn(B, H * W * 3, 5 + C, generator=g)
    return lg, dout, [30.0, 61.0, 62.0, 45.0, 59.0, 119.0], 16.0


@pytest.mark.parametrize("math", ["f32", "bf16"])
@pytest.mark.parametrize("cout", TRAIN_COUTS)
def test_training_head_references_meet_conv_bar(cout, math):
    """Forward (+ bias), dgrad and wgrad of the training head at cout > 256: the fp32-rounded float64 result against train_kernel_ref.CONV_BAR."""
    case = train_case(cout)
    d = te.conv_case_data(case, math == "bf16")
    for name, (ref, sc) in (("fwd", K.conv_fwd(d["x64"], d["w64"], 1, d["bias"].double())), ("dgrad", K.conv_dgrad(d["x64"].shape, d["w64"], d["dz64"], 1)),
                            ("wgrad", K.conv_wgrad(d["x64"], d["w64"].shape, d["dz64"], 1))):
        assert K.conv_ratio(ref.float(), ref, sc) <= 1.0, (cout, math, name)
    for P in (1, 338):
        dl = torch.randn(P, cout, generator=torch.Generator().manual_seed(P * 3 + cout))
        _, rb_, ra = K.bias_bwd(dl.double(), -1.75)
        assert K.ratio(rb_.float(), rb_, K.BN_BAR * ra + 1e-30) <= 1.0


@pytest.mark.parametrize("C,same_cell", [(C, False) for C in LOSS_CLASSES] + [(123, True)])
def test_loss_cases_clear_the_margins(C, same_cell):
    spec, x, tg, res = loss_case(C, same_cell)
    assert tuple(x.shape) == (2, cout_of(C), 8, 8) and res["nGT"] >= 1 and R.margins_ok(res["margins"])
    if same_cell:                             # both rows on one cell of this head: tcls is the union of their classes
        cells = R._obj_cells(x, tg, spec)
        first = [c[:4] for c in cells if c[0] == 0][:2]
        assert len(first) == 2 and first[0] == first[1], first
        assert int(tg[0, 0, 0]) != int(tg[0, 1, 0]) and int(tg[0, 1, 0]) == C - 1 and 5 + C >= 128


# ----------------------------------------------------------------------------- the whole-step draw (C = 81, 96 x 96, B = 2)
# The whole-step criterion of tests/test_gpu_train.py holds every tensor to 16 x the worst error of ONE fp32 run on the CPU.  At this size a
# train-mode step has, on every draw, a few LeakyReLU decisions that fp32 cannot make: pre-activations u closer to 0 than fp32's own error
# at that layer (delta = max |u_fp32 - u_float64| of the CPU run, 3e-5 .. 1e-4 behind 60 layers), in layers of 18 .. 72 pixels where ONE such
# element carries 5 - 8 % of a BatchNorm bias gradient.  Whether the bar is above that movement depends on whether the CPU run itself took one
# of those decisions the other way -- not on the code under test.  So the draw is picked as the loss targets are (pick_target: no ambiguous
# decision), from the two CPU references alone: the first image seed from 31 upwards on which the largest movement a single ambiguous
# decision (|u_float64| <= 4 delta) can cause, 0.9 |dy| / ||dbeta||, is at most a quarter of the bar.  Measured (seed: 16 x worst fp32 error,
# largest ambiguous movement / bar): 31: 0.0305, 2.5 | 32: 0.098, 0.55 | 33: 0.0082, 10 | 34: 0.15, 0.51 | 35: 0.99, 0.07 | 36: 0.00016, 369 |
# 37: 0.15, 0.37 | 38: 0.22 .. 0.54 (thread count), 0.24 .. 0.10.  Seed 31 holds the element the GPU decides the other way: u = -1.04e-5 in
# pre_det2.mlist.1 (the CPU's fp32 run has -1.33e-5 there and is off by 1e-5 two elements further), movement 0.0346 against a bar of 0.0305.
# The price: on such a draw the whole-step bar is coarse (tests/test_gpu_train_local.py says so of every whole-step test); the strict check of
# the step is the op-by-op one, which runs on seed 31.
STEP_IMAGES_SEED = 35
STEP_AMBIGUOUS = 4.0          # |u| <= STEP_AMBIGUOUS * delta: a decision fp32 may take either way
STEP_MARGIN = 0.25            # largest single ambiguous movement <= STEP_MARGIN * bar


def step_draw_figures(seed, C=81, size=96, B=2):
    """(bar = 16 x the worst per-tensor error of torch's fp32 step, the largest movement of a BatchNorm bias gradient one ambiguous LeakyReLU
    decision can cause) of the F32 train-mode step on synth.images(B, size, seed), from the float64 and the fp32 CPU runs of tests/train_ref."""
    from tests import test_gpu_train as gt, train_ref as T
    from tests.helpers import trained_like_stream
    from yolo_v3_amd import YoloNet, WeightManager
    net = YoloNet((size, size), numClass=C)
    WeightManager(net).load_stream(trained_like_stream(C))
    sd = {k: v.detach().clone() for k, v in net.train().state_dict().items()}
    x = torch.from_numpy(np.ascontiguousarray(synth.images(B, size, seed)))
    tg = gt.pick_target(T.forward(sd, x, True)[0], size, C, B, 8, 77)
    plain = T.F.leaky_relu

    def run(dtype):
        seen = []

        def recording(u, slope):
            u.retain_grad()
            seen.append(u)
            return plain(u, slope)
        T.F.leaky_relu = recording
        try:
            return T.run(sd, x, tg, C, train=True, dtype=dtype), seen
        finally:
            T.F.leaky_relu = plain
    r64, u64 = run(torch.float64)
    r32, u32 = run(torch.float32)
    bar = gt.BAR_FACTOR * max(T.rel_l2(r32["grads"][k], g) for k, g in r64["grads"].items())
    worst = 0.0
    for a, b in zip(u64, u32):
        u, g = a.detach(), a.grad                                    # g = dy * slope(u)
        delta = float((b.detach().double() - u).abs().max())
        dy = g / torch.where(u > 0, torch.ones_like(u), torch.full_like(u, K.SLOPE))
        move = (1 - K.SLOPE) * dy.abs() / g.sum((0, 2, 3)).norm()
        amb = u.abs() <= STEP_AMBIGUOUS * delta
        if bool(amb.any()):
            worst = max(worst, float(move[amb].max()))
    return bar, worst


def test_whole_step_draw_has_its_bar_above_every_ambiguous_decision():
    bar, worst = step_draw_figures(STEP_IMAGES_SEED)
    print("seed %d: bar %.3g, largest movement of one ambiguous LeakyReLU decision %.3g (%.2f of the bar)" % (STEP_IMAGES_SEED, bar, worst, worst / bar))
    assert 0.0 < worst <= STEP_MARGIN * bar


# ----------------------------------------------------------------------------- 3. selection
@functools.lru_cache(maxsize=None)
def _recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_select_wide_heads.json")) as f:
        return json.load(f)


def test_wide_head_selection_matches_the_recorded_table():
    want, lib = _recorded(), _ffi.lib()
    assert want["cus"] == 256
    keys = ["%s/%d/%d" % (cfg, C, B * 169) for cfg in grid.WIDE_HEAD_CONFIGS for C in grid.WIDE_HEAD_CLASSES for B in grid.WIDE_HEAD_BATCHES]
    assert sorted(keys) == sorted(want["heads"]) and set(grid.WIDE_HEAD_CLASSES) == set(CLASSES)
    assert {338, 5408} <= {B * 169 for B in grid.WIDE_HEAD_BATCHES}
    diff = []
    for cfg in grid.WIDE_HEAD_CONFIGS:
        for C in grid.WIDE_HEAD_CLASSES:
            for B in grid.WIDE_HEAD_BATCHES:
                d = grid.wide_head_desc(lib, cfg, C, B)
                assert d.cout == cout_of(C) and d.cout_pad == cout_pad_of(d.dtype, d.cout) and d.B * d.H * d.W == B * 169
                got, rec = grid.query(lib, d), grid.parse(want["heads"]["%s/%d/%d" % (cfg, C, B * 169)], want["kernels"])
                if got != rec:
                    diff.append("%s C=%d M=%d: form, launches, kernel %s, recorded %s" % (cfg, C, B * 169, got, rec))
    assert not diff, "\n".join(diff)


def test_gemm_form_at_wide_heads():
    """Exact fp32: C = 123 (cout = cout_pad = 384 = 3 x 128) takes the persistent GEMM once its 128 x 128 tiles fill one round of the 256 CUs
    (M = 10985: 86 x 3 = 258 tiles; 5408 rows give 129) -- two launches, the rest of the rows on the 64x64 tiles -- and at any M when forced;
    C = 81 (cout 258: neither a multiple of 64 nor its own padding) never does, forced or not.  The tile counts of every mode: ceil(cout / 128)
    channel tiles in the plane modes, cout_pad / 32 (or / 64 at 384) in exact fp32."""
    want = _recorded()
    ans = {k: grid.parse(t, want["kernels"]) for k, t in want["heads"].items()}
    form, launches, line = ans["f32/123/10985"]
    assert (form, launches) == (0, 2) and line.startswith("GEMM_128x128 nt=3 ") and "rows=10880 grid=256 rest 64x64 nt=6" in line
    assert ans["f32/123/5408"][2].startswith("64x64 nt=6") and ans["f32/123/338"][2].startswith("64x64 nt=6")
    for M in (338, 5408):
        assert ans["f32.tune0=14/123/%d" % M][2].startswith("GEMM_128x128 nt=3 ") and ans["f32.tune0=14/123/%d" % M][1] == 1
    for key, (form, launches, line) in ans.items():
        cfg, C, M = key.split("/")
        assert form == 0
        if C == "81" or cfg == "f32.tune0=13":
            assert "GEMM" not in line and launches == 1, (key, line)
        nt = int(line.split("nt=")[1].split()[0])
        if cfg.startswith("f32") and cfg not in ("f32h2", "f32x3"):
            assert line.startswith("GEMM") or nt == {"81": 9, "82": 9, "91": 9, "123": 6, "166": 17, "300": 29}[C], (key, line)
        else:
            assert nt == -(-cout_of(int(C)) // 128) >= 3, (key, line)
