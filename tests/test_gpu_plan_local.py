"""Every launch of the exact-fp32 plans the benchmark times, against float64 on the GPU's OWN inputs (-m gpu, through the C-ABI).

`Plan` gives every conv its own output buffer, so after one forward all outputs and all inputs are still on the device.  For each launch:

  * float64 truth (tests/plan_ref.py: BatchNorm folded in float64 from the module's parameters) on conv_ref.sample_rows -- every border of
    image 0, the first and last pixel of every image, the last 256 rows, 2048 random rows; every row of launches up to 8192 rows -- computed
    from the input tensors read back from the GPU, so errors do not compound; nothing excluded;
  * the FULL tensor against an independent launch path of a copy of the plan's own descriptor, written into a NaN-filled buffer with a NaN
    canary behind it on the plan's own Winograd scratch: Winograd launches against the direct tiles (w_wino = w_wino4 = NULL) and, F(4x4),
    against one item per workgroup (tune[1] = 1: another summation order where the even schedule cut items); plain 1x1 launches
    (persistent GEMM + tiles split) against the tiles alone (tune[0] = 13) and every other direct launch against the 64x64 tiles
    (tune[0] = 2): documented same K order, bit-identical.  Every element written, canary intact, status word 0.  This is what catches a
    fault confined to one item of a ragged last round;
  * the fused front kernels (feature.mlist.0 + .1; the first residual block), whose intermediates are never materialised: against float64
    from the image / from the GPU's feature.mlist.1, and bit for bit against the un-fused launches of the plan's own descriptors;
  * the three heads' logits like every launch; the detections tensor == yv3_decode of those logits, bit for bit;
  * the descriptor's input pointers name the producers plan_ref.network_graph (written from the reference's wiring) expects.

Bars.  The fused front kernels (K = 27 ... 288) are held to the project's fixed exact-fp32 bar, |got - ref| <= 2e-5 * max(1, |ref|)
(tests/test_gpu_conv_matrix.py).  For the yv3_conv2d launches that bar does not fit real activations: on the first run the K = 4608 layers at
13x13 were 1.9 x (3x3 stride 2, direct tiles) and 2.1 x (F(4x4)) that bar away from float64 and a K = 1024 1x1 layer 1.06 x -- where torch's
own fp32 convolution on the CPU, same rows of the same inputs, was 1.9 x / 2.4 x / 1.0 x away, and the independent paths agreed.  So each
launch's bar is a multiple of what the reference's arithmetic itself loses: DIRECT_X = 4 x (direct forms), WINO_X = 8 x (Winograd forms:
about 2 x per Winograd layer, the rest is margin for summation order) the error of torch fp32 on the CPU against float64 on the same
sampled rows (never taken below one fp32 rounding, 2^-24).  Full tensor: Winograd vs direct within 12 x (triangle inequality), even
schedule vs one item per workgroup within the launch's own bar.  The code under test never sets its bar.
Measured (MI355X, 256 CUs), worst sampled error per launch class over the five plans, in units of the fixed 2e-5 bar | of torch fp32's error:
Winograd F(4x4) 2.08 | 1.8 (pre_det1.mlist.3, one lane of 64); direct tiles 1.91 | 1.2 (feature.mlist.24, dense); plain 1x1 1.06 | 1.15
(pre_det1.mlist.0); 1x1 GEMM + tiles 0.89; fused front 0.07, fused res64 0.035.  Full tensor: Winograd vs direct 2.7 x the fixed bar (dense,
pre_det1.mlist.1); even schedule vs one item per workgroup 0.06 x; GEMM + tiles vs tiles, tiles vs 64x64 tiles, fused vs un-fused: bit-identical.
"""
import ctypes
import time

import pytest
import torch

from yolo_v3_amd import _ffi, synth, Detector, YoloNet, WeightManager
from tests import conv_ref as cr
from tests import plan_ref as pr
from tests.helpers import load_sw1_net, desc_inputs_by_pointer, copy_desc, relaunch_desc

pytestmark = pytest.mark.gpu

F32 = _ffi.F32
BAR = pr.BAR                # the fused front kernels (K = 27 ... 288): the project's fixed exact-fp32 bar
DIRECT_X, WINO_X = 4, 8     # yv3_conv2d launches: multiples of torch fp32's own error on the same rows (direct forms / Winograd forms)
FP32_ULP = 2.0 ** -24       # ... which is never taken below one fp32 rounding of the result
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    yield
    torch.cuda.synchronize()


_copy, _relaunch = copy_desc, relaunch_desc      # (shared with tests/test_gpu_plane_plan_local.py: tests/helpers.py)


def _dev_err(a, b):
    """max |a - b| / max(1, |b|) of two device tensors, and the flat index of the worst element."""
    e = (a.double() - b.double()).abs() / b.double().abs().clamp(min=1.0)
    i = int(e.argmax())
    return float(e.reshape(-1)[i]), i


def _check_plan(eng, plan, x, dets, params, graph, label):
    """All checks of one plan after its forward.  x: the plan's images (device, NCHW); dets: the [B, N, 5+C] rows its decode wrote."""
    t0 = time.time()
    lib = _ffi.lib()
    names = desc_inputs_by_pointer(plan)
    by_name = {n.name: n for n in graph}
    B, H, W = plan.B, plan.H, plan.W
    assert plan.fused_front and plan.fused_res64 and plan.first_desc == 3
    torch.cuda.synchronize()
    assert int(plan.flags.item()) == 0, "%s: status word %d after the forward" % (label, int(plan.flags.item()))
    fails, table = [], []                                      # table: (error / bar, class, launch index, name, error / 2e-5, error / torch fp32's)

    def host(name):
        return plan.layer_out[name].cpu() if name is not None else None

    def sampled(name, ref, rows, cls, j, bar=BAR, t32=None):
        out = plan.layer_out[name]
        got = out.reshape(-1, out.shape[-1])[rows.cuda()].cpu()
        assert bool(torch.isfinite(got).all()), "%s %s: non-finite output" % (label, name)
        e = pr.norm_err(got, ref)
        r = float(e.max()) / bar
        table.append((r, cls, j, name, float(e.max()) / BAR, float(e.max()) / t32 if t32 else 0.0))
        if r > 1.0:
            row, ch = divmod(int(e.argmax()), e.shape[1])
            fails.append("%s launch %d %s [%s]: %.3g x its bar (%.3g) vs float64 at output row %d channel %d" % (
                label, j, name, cls, r, bar, int(rows[row]), ch))
        return r

    # ---- the fused front kernels: float64 from what they read, and bit for bit against the un-fused launches
    g0, g1, g2, g3 = graph[:4]
    img = x.cpu().permute(0, 2, 3, 1)
    h1, w1 = H // 2, W // 2
    rows = pr.rows_of(B, h1, w1, seed=1)
    sampled(g1.name, pr.fused_pair_ref(g0, params[g0.name], g1, params[g1.name], img, rows), rows, "fused front", 0)
    m1 = host(g1.name)
    rows = pr.rows_of(B, h1, w1, seed=2)
    sampled(g3.name, pr.fused_pair_ref(g2, params[g2.name], g3, params[g3.name], m1, rows, residual=m1), rows, "fused res64", 2)
    del img
    assert [names(plan.descs[j]) for j in range(3)] == [(g.x, g.x2, g.residual) for g in (g1, g2, g3)]
    eng.run_conv0(plan, x)
    y1 = _relaunch(_copy(plan.descs[0]), B * h1 * w1 * 64, "%s un-fused %s" % (label, g1.name))
    assert torch.equal(y1, plan.layer_out[g1.name].reshape(-1)), "%s: fused front differs from the two-launch path in %d elements" % (
        label, int((y1 != plan.layer_out[g1.name].reshape(-1)).sum()))
    _ffi.check(lib.yv3_conv2d(ctypes.byref(plan.descs[1]), _ffi.stream_ptr()), "un-fused " + g2.name)
    y3 = _relaunch(_copy(plan.descs[2]), B * h1 * w1 * 64, "%s un-fused %s" % (label, g3.name))
    assert torch.equal(y3, plan.layer_out[g3.name].reshape(-1)), "%s: fused res64 differs from the two-launch path in %d elements" % (
        label, int((y3 != plan.layer_out[g3.name].reshape(-1)).sum()))
    del y1, y3, m1

    # ---- every launch of the sequence
    forms = plan.forms()
    nl = plan.launches()
    second = {"wino vs direct": (0.0, None), "F(4x4) even vs one item per workgroup": (0.0, None)}
    n_split = n_cut = 0
    for j in range(plan.first_desc, plan.n_desc):
        d = plan.descs[j]
        si, f = forms[j - plan.first_desc]
        assert si == plan.desc_spec[j]
        name = eng.specs[si].name
        node = by_name[name]
        assert names(d) == (node.x, node.x2, node.residual) and d.cin_up == node.cin_up, (name, names(d))
        ho, wo = cr.out_hw(d.H, d.W, d.k, d.stride)
        out = plan.layer_out[name]
        n = B * ho * wo * d.cout
        assert d.B == B and out.numel() == n and out.data_ptr() == d.y
        plain = d.k == 1 and not d.residual and not d.cin_up and d.cout % 64 == 0
        cls = {0: "1x1 GEMM + tiles" if plain and nl[j - plan.first_desc] == 2 else "1x1 plain" if plain else "direct tiles",
               1: "Winograd F(2x2)", 2: "Winograd F(4x4)"}[f]
        rows = pr.rows_of(B, ho, wo, seed=j)
        ins = (host(node.x), host(node.x2), host(node.residual))
        ref = pr.launch_ref(node, params[name], *ins, pixels=rows)
        # this launch's bar: a multiple of what the reference's own arithmetic (torch fp32 on the CPU) loses on the same rows of the same inputs
        t32 = max(float(pr.norm_err(pr.torch_f32_rows(node, params[name], *ins, pixels=rows), ref).max()), FP32_ULP)
        bar = (WINO_X if f != 0 else DIRECT_X) * t32
        del ins
        sampled(name, ref, rows, cls, j, bar, t32)
        what = "%s launch %d %s [%s]" % (label, j, name, cls)
        flat = out.reshape(-1)
        c = _copy(d)
        if f != 0:
            c.w_wino, c.alpha_wino, c.w_wino4 = None, None, None
            assert lib.yv3_conv2d_form(ctypes.byref(c)) == 0
            e, i = _dev_err(_relaunch(c, n, what + " as direct tiles"), flat)
            if e / t32 > second["wino vs direct"][0]:
                second["wino vs direct"] = (e / t32, what)
            if e > (WINO_X + DIRECT_X) * t32:                      # (triangle inequality: each side within its bar of float64)
                fails.append("%s: %.3g x torch fp32's error against the direct tiles at element %d (bound %d x)" % (what, e / t32, i, WINO_X + DIRECT_X))
            if f == 2:
                c = _copy(d)
                c.tune[0], c.tune[1] = 11, 1                      # F(4x4) whatever the item count, one item per workgroup
                assert lib.yv3_conv2d_form(ctypes.byref(c)) == 2
                y = _relaunch(c, n, what + ", one item per workgroup")
                n_cut += not torch.equal(y, flat)
                e, i = _dev_err(y, flat)
                if e / t32 > second["F(4x4) even vs one item per workgroup"][0]:
                    second["F(4x4) even vs one item per workgroup"] = (e / t32, what)
                if e > bar:
                    fails.append("%s: %.3g x its bar against one item per workgroup at element %d" % (what, e / bar, i))
        else:
            n_split += cls == "1x1 GEMM + tiles"
            c.tune[0] = 13 if plain else 2
            y = _relaunch(c, n, what + ", tune[0] = %d" % c.tune[0])
            if not torch.equal(y, flat):
                e, i = _dev_err(y, flat)
                fails.append("%s: %d elements differ from the tiles (tune[0] = %d), worst %.3g x the bar at element %d" % (
                    what, int((y != flat).sum()), c.tune[0], e / BAR, i))

    # ---- decode: the detections are yv3_decode of the plan's logits
    again = torch.full_like(dets, NAN)
    eng.run_decode(plan, again)
    torch.cuda.synchronize()
    assert torch.equal(again, dets), "%s: detections differ from yv3_decode of the plan's logits" % label
    assert int(plan.flags.item()) == 0, "%s: status word %d" % (label, int(plan.flags.item()))

    by_cls = {}
    for r, cls, j, name, rb, rt in table:
        c = by_cls.setdefault(cls, [0.0, 0.0, 0.0, None])
        c[1], c[2] = max(c[1], rb), max(c[2], rt)
        if r >= c[0]:
            c[0], c[3] = r, name
    r, cls, j, name, rb, rt = max(table)
    print("plan %s: worst error / bar %.3f at launch %d %s [%s] over %d launches (%d F(4x4), %d of them not bit-equal to one item per workgroup: "
          "items cut by the even schedule; %d 1x1 launches split GEMM + tiles); %.0f s" % (
              label, r, j, name, cls, len(table), sum(f == 2 for _, f in forms), n_cut, n_split, time.time() - t0))
    print("    per class, worst error / its bar | / 2e-5 | / torch fp32's error: " + "; ".join(
        "%s %.3f | %.3f | %.2f (%s)" % (k, v[0], v[1], v[2], v[3]) for k, v in sorted(by_cls.items())))
    print("    second path, full tensor, in units of torch fp32's error on the sampled rows: " + "; ".join("%s %.3f" % (k, v[0]) for k, v in second.items()))
    return fails


@pytest.fixture(scope="module")
def sw1(sw1_stream):
    net = load_sw1_net(sw1_stream)
    params = pr.fold_params(net)
    return net.cuda(), params, pr.network_graph()


@pytest.mark.parametrize("lanes", [2, 1])
def test_headline_plans_launch_by_launch(sw1, lanes):
    """bench.py's headline (416x416 bs=64, ``synth.images(64, 416, 1000)``, exact fp32) as two lanes of 32 -- BOTH lane plans, after they
    ran concurrently: lane 1 is where a cross-lane race on flags or scratch would show -- and as one lane of 64."""
    net, params, graph = sw1
    x = torch.from_numpy(synth.images(64, 416, 1000)).cuda()
    det = Detector(net, 64, 416, 416, 0.5, 0.4, dtype=F32, lanes=lanes)
    assert det.lanes == lanes
    with torch.no_grad():
        det(x)
    fails = []
    for i, (p, off) in enumerate(zip(det.lane_plans, det.lane_off)):
        assert p.B == 64 // lanes
        fails += _check_plan(det.engine, p, x[off:off + p.B], det.dets[off:off + p.B], params, graph, "416x416 bs=64 lane %d of %d" % (i, lanes))
    assert not fails, "\n".join(fails)


def _forward_and_check(net, params, graph, x, label):
    eng = net.engine(F32)
    with torch.no_grad():
        dets, plan = eng.forward(x)
    fails = _check_plan(eng, plan, x, dets, params, graph, label)
    assert not fails, "\n".join(fails)


def test_dense_608_bs8_plan_launch_by_launch():
    """bench.py's dense config: 608x608 bs=8 on the SW-dense weights."""
    net = load_sw1_net(synth.dense_weight_stream(), 608)
    params = pr.fold_params(net)
    _forward_and_check(net.cuda(), params, pr.network_graph(), torch.from_numpy(synth.images(8, 608, 4)).cuda(), "608x608 bs=8 dense")


def test_one_image_plan_launch_by_launch(sw1):
    """416x416 bs=1: the even schedule on every F(4x4) launch, no whole rounds anywhere."""
    net, params, graph = sw1
    _forward_and_check(net, params, graph, torch.from_numpy(synth.images(1, 416, 1000)).cuda(), "416x416 bs=1")


def test_non_square_plan_launch_by_launch(sw1_stream):
    """320 (H) x 480 (W), bs=3: pictures of 10x15 ... 80x120 cells, sides that are not multiples of the 4x4 tile grid."""
    net = YoloNet((480, 320)).eval()
    assert WeightManager(net).load_stream(sw1_stream) == sw1_stream.size
    params = pr.fold_params(net)
    x = torch.from_numpy(synth.images(3, 480, 1003)[:, :, :320, :480].copy()).cuda()
    _forward_and_check(net.cuda(), params, pr.network_graph(), x, "320x480 bs=3")
