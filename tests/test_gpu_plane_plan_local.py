"""Every launch of the smallest plane-mode plans that reach the kernels -- F32H2 (two fp16 planes, the default mode), F32X3 (what a saturated
batch is re-run in), BF16 -- against float64 on the GPU's OWN inputs (-m gpu, through the C-ABI), as tests/test_gpu_plan_local.py does for
exact fp32.  The bar is tests/plane_bar.py's (derived beforehand, checked without a GPU by tests/test_plane_bar_host.py):

  * wiring: the descriptor's input pointers name the producers plan_ref.network_graph expects;
  * value: bars 1 and 2 in units of 2^-24 * mag (+ 2^-25 for stored fp16 planes) on plan_ref.rows_of against plan_ref.launch_ref on the
    tensors read back through engine.from_planes, torch fp32 on the same rows as bar 2's yardstick; check 3 (the stored planes are a
    nearest split) on the full tensor on the device; every value finite.  BF16: conv_ref.bf16_report (criteria A and B, bf16-rounded
    weights), heads conv_ref.F32_BAR;
  * independent path: a copy of the descriptor relaunched into a NaN-filled buffer of the same plane layout with a NaN canary behind it
    (every element written, canary intact, status word 0): stream-K launches without the workspace (within twice the launch's bar, full
    tensor), Winograd launches as direct tiles (form 0 asserted; within (WINO_X + DIRECT_X) x torch's error, full tensor), every other launch
    with forced tile code 2 and no workspace: bit-identical;
  * the fused front and first residual block: their un-fused launches of the plan's own descriptors on the device's tensors, each against
    float64 with bars 1 to 3; the fused kernels' outputs equal them bit for bit;
  * the fused-decode heads: each head descriptor relaunched with dec_out = NULL into a fresh fp32 buffer, logits against float64 (bars 1
    and 2 without the 2^-25), yv3_decode of them == the plan's rows of the detections tensor, bit for bit;
  * after the plan: status word 0, every stream-K hand-over flag consumed.
The plan itself is asserted through plan.kernels() / forms() / launches() against tests/golden/conv_select_256cu.json on 256 CUs.
Not reached by these plans (they need 32 to 64 images per lane; they stay with the kernel-level tests): W4_192x128 nt=8, WINO_PINGPONG nt=8,
256x128_W8 nt=8.
"""
import ctypes
import json
import os
import time

import pytest
import torch

from oracle import oracle_cpu as oc
from yolo_v3_amd import _ffi, engine, synth, Detector, YoloNet, WeightManager
from tests import conv_ref as cr
from tests import conv_select_grid as grid
from tests import plan_ref as pr
from tests import plane_bar as pb
from tests.helpers import load_sw1_net, desc_inputs_by_pointer, copy_desc, relaunch_desc

pytestmark = pytest.mark.gpu

F32, BF16, F32X3, F32H2 = _ffi.F32, _ffi.BF16, _ffi.F32X3, _ffi.F32H2
NAN = float("nan")
FORCED = _ffi.TILE_128x128_W8 << _ffi.OPT_TILE_SHIFT
SK_FLAG_BYTES = 4 * 512                    # the hand-over flags at the end of the stream-K workspace


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def select_table(golden_dir):
    with open(os.path.join(golden_dir, "conv_select_256cu.json")) as f:
        return json.load(f)


def _assert_plan_is_the_tables(plan, table, key, label):
    """plan.kernels() / forms() / launches() == the golden selection table's row `key` (256 CUs; printed on any other CU count)."""
    kernels, forms, launches = plan.kernels(), plan.forms(), plan.launches()
    print("plan %s reaches: %s" % (label, "; ".join(sorted(set(kernels)))))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if key is None or cus != table["cus"]:
        print("plan %s: not compared with the selection table (%s, %d CUs)" % (label, key, cus))
        return kernels
    layer_of = [int(t) for t in table["layer_of"][key.split("/")[1]].split()]
    tokens = table["layers"][key].split()
    for i, j in enumerate(range(plan.first_desc, plan.n_desc)):
        want = grid.parse(tokens[layer_of[plan.desc_spec[j]]], table["kernels"])
        assert (forms[i][1], launches[i], kernels[i]) == want, "%s descriptor %d: %s, the table's %s has %s" % (
            label, j, (forms[i][1], launches[i], kernels[i]), key, want)
    return kernels


def _check_plan(eng, plan, x, dets, params, graph, label, kernels, which="all"):
    """All checks of one plan after its forward.  x: the plan's images (device, NCHW); dets: the [B, N, 5+C] rows its heads wrote.
    which: "all" launches, the first launch of each "distinct" layer (conv_select_grid.classes), or "wino" (Winograd launches only); the
    heads always; the fused front's un-fused launches unless "wino"."""
    t0 = time.time()
    lib, mode = _ffi.lib(), eng.dtype
    NP = engine.PLANES[mode]
    store = {F32H2: torch.float16, F32X3: torch.bfloat16, BF16: torch.bfloat16}[mode]
    names = desc_inputs_by_pointer(plan)
    by_name = {n.name: n for n in graph}
    B, H, W = plan.B, plan.H, plan.W
    assert plan.fused_decode and len(plan.head_descs) == 3
    torch.cuda.synchronize()
    assert int(plan.flags.item()) == 0, "%s: status word %d after the forward" % (label, int(plan.flags.item()))
    fails, table = [], []                          # table: (class, name, units, units / torch's, error / 2e-5) -- BF16: (class, name, worst / eps, share, 0)
    img = x.cpu().permute(0, 2, 3, 1).contiguous()

    def host(name):
        if name is None:
            return None
        return img if name == pr.IMAGE else engine.from_planes(plan.layer_out[name], mode).cpu()

    def p_of(node):
        p = params[node.name]
        return p._replace(w=oc.round_bf16(p.w)) if (mode == BF16 and node.spec.cin != 3) else p

    def value(out, node, ins, rows, cls, what, planes=NP, wino=False):
        """Bars 1 and 2 (BF16: criteria A and B) of device tensor `out` ([planes][M, cout], any shape) on `rows`, check 3 on all of it.
        Returns (torch fp32's error in units, the tighter of bars 1 and 2 in units)."""
        p, C = p_of(node), node.spec.cout
        flat = out.reshape(planes, -1, C)
        assert bool(torch.isfinite(flat).all()), "%s: non-finite output" % what
        got = flat[:, rows.cuda()].double().sum(0).cpu()
        ref = pr.launch_ref(node, p, *ins, pixels=rows)
        mag = cr.conv_desc_mag(ins[0], p.w, p.beta, p.alpha, ins[2], ins[1], node.cin_up, node.spec.stride, pixels=rows)
        K = node.spec.k ** 2 * node.spec.cin
        if mode == BF16:
            if out.dtype == torch.float32:
                e = float(pr.norm_err(got, ref).max())
                table.append((cls, node.name, e / cr.F32_BAR, 0.0, e / pb.OLD_BAR))
                if e > cr.F32_BAR:
                    fails.append("%s: fp32 logits %.3g x the 2e-5 bar from float64" % (what, e / cr.F32_BAR))
            else:
                r = cr.bf16_report(got, ref, mag, K)
                table.append((cls, node.name, r["worst"], r["share"], 0.0))
                if not (r["a_ok"] and r["b_ok"]):
                    fails.append("%s: BF16 bar: %d elements outside their interval (first %s), share of got != bf16(ref) %.3g (cap %.1g)" % (
                        what, r["outside"], r["first"], r["share"], cr.BF16_SHARE_CAP))
            return 1.0, 1.0
        t32 = pr.torch_f32_rows(node, params[node.name], *ins, pixels=rows)
        v = pb.judge(got, ref, mag, t32, K, wino, fp16_planes=(mode == F32H2 and planes == 2))
        table.append((cls, node.name, v.units, v.units / max(v.torch, 1.0), v.old))
        if not (v.ok1 and v.ok2):
            fails.append("%s [%s]: %.3g units from float64 at row %d channel %d (bar 1 %.3g, bar 2 %.3g = %d x torch fp32's %.3g; %.3g x the 2e-5 bar)" % (
                what, cls, v.units, int(rows[v.at[0]]), v.at[1], v.bar1, v.bar2, pb.WINO_X if wino else pb.DIRECT_X, v.torch, v.old))
        if planes > 1:
            bad = pb.split_violations(out.reshape(planes, -1))
            if bad:
                fails.append("%s: %d of %d stored elements are not a nearest split (check 3)" % (what, bad, flat[0].numel()))
        return max(v.torch, 1.0), min(v.bar1, v.bar2)

    def equal_bits(a, b, what):
        if not torch.equal(a.reshape(-1), b.reshape(-1)):
            fails.append("%s: %d elements differ" % (what, int((a.reshape(-1) != b.reshape(-1)).sum())))

    # ---- the front: feature.mlist.0 alone, and (fused plans) the un-fused launches of the plan's own descriptors, bit for bit against the fused kernels
    g0, g1, g2, g3 = graph[:4]
    if which != "wino":
        if plan.fused_front:
            assert plan.fused_res64 and plan.first_desc == 3
            assert [names(plan.descs[j]) for j in range(3)] == [(g.x, g.x2, g.residual) for g in (g1, g2, g3)]
            eng.run_conv0(plan, x)
        else:
            assert plan.first_desc == 0
        value(plan.conv0_out, g0, (img, None, None), pr.rows_of(B, H, W, seed=100), "conv0", "%s yv3_conv0 %s" % (label, g0.name))
        if plan.fused_front:
            h1, w1 = H // 2, W // 2
            n1 = B * h1 * w1 * 64
            m0 = host(g0.name)
            y1 = relaunch_desc(copy_desc(plan.descs[0]), n1, "%s un-fused %s" % (label, g1.name), store, NP)
            value(y1, g1, (m0, None, None), pr.rows_of(B, h1, w1, seed=101), "un-fused front", "%s un-fused %s" % (label, g1.name))
            equal_bits(y1, plan.layer_out[g1.name], "%s: fused front vs the two-launch path" % label)
            del m0
            m1 = host(g1.name)
            _ffi.check(lib.yv3_conv2d(ctypes.byref(plan.descs[1]), _ffi.stream_ptr()), "un-fused " + g2.name)
            value(plan.layer_out[g2.name], g2, (m1, None, None), pr.rows_of(B, h1, w1, seed=102), "un-fused res64", "%s un-fused %s" % (label, g2.name))
            y3 = relaunch_desc(copy_desc(plan.descs[2]), n1, "%s un-fused %s" % (label, g3.name), store, NP)
            value(y3, g3, (host(g2.name), None, m1), pr.rows_of(B, h1, w1, seed=103), "un-fused res64", "%s un-fused %s" % (label, g3.name))
            equal_bits(y3, plan.layer_out[g3.name], "%s: fused res64 vs the two-launch path" % label)
            del y1, y3, m1

    # ---- the launches of the sequence
    forms = plan.forms()
    layer_class = grid.classes(416)[1]
    heads = {di: k for k, (di, _, _) in enumerate(plan.head_descs)}
    again = torch.full_like(dets, NAN)
    seen, second = set(), {"stream-K vs no workspace": 0.0, "Winograd vs direct": 0.0}
    n_sk = n_wino = n_checked = 0
    for i, j in enumerate(range(plan.first_desc, plan.n_desc)):
        d = plan.descs[j]
        si, f = forms[i]
        assert si == plan.desc_spec[j]
        name = eng.specs[si].name
        node = by_name[name]
        assert names(d) == (node.x, node.x2, node.residual) and d.cin_up == node.cin_up, (name, names(d))        # wiring: every launch
        head, sk = j in heads, " sk" in kernels[i]
        assert not (f and sk) and f in (0, 1) and not (head and (f or sk))
        first = layer_class[si] not in seen
        seen.add(layer_class[si])
        if not (head or which == "all" or (which == "distinct" and first) or (which == "wino" and f == 1)):
            continue
        n_checked += 1
        ho, wo = cr.out_hw(d.H, d.W, d.k, d.stride)
        n = B * ho * wo * d.cout
        assert d.B == B
        cls = ("head " if head else "") + kernels[i].split()[0] + (" sk" if sk else "")
        what = "%s launch %d %s [%s]" % (label, j, name, kernels[i])
        rows = pr.rows_of(B, ho, wo, seed=j)
        ins = (host(node.x), host(node.x2), host(node.residual))
        c = copy_desc(d)
        if head:
            # the logits are never materialised: relaunch with dec_out = NULL into a fresh fp32 buffer, decode them with yv3_decode
            assert d.y is None and d.dec_out and d.out_dtype == F32
            c.dec_out = None
            out = relaunch_desc(c, n, what + ", dec_out = NULL")
            value(out, node, ins, rows, cls, what, planes=1)
            anc, stride, row0, _, hh, ww = plan.decode_args[heads[j]]
            assert (hh, ww) == (ho, wo)
            _ffi.check(lib.yv3_decode(out.data_ptr(), d.cout, anc, stride, again.data_ptr() + row0 * plan.attrib * 4, plan.N * plan.attrib,
                                      B, hh, ww, eng.num_class, _ffi.stream_ptr()), "yv3_decode")
            c = copy_desc(c)
            planes, dt = 1, torch.float32
        else:
            out = plan.layer_out[name]
            assert out.numel() == NP * n and out.data_ptr() == d.y
            t32u, bar = value(out, node, ins, rows, cls, what, wino=f == 1)
            planes, dt = NP, store
        if sk or f == 1:
            # another summation order: the full tensor in units, u from fp32 mag of every element
            u = pb.unit(pb.mag_f32(node, params[name], *ins), mode == F32H2).cuda()
            if sk:
                n_sk += 1
                c.workspace, c.workspace_bytes = None, 0
                assert " sk" not in _ffi.conv2d_kernel(c)
                bound, key, other = 2.0 * bar, "stream-K vs no workspace", "without the workspace"
            else:
                n_wino += 1
                c.w_wino, c.alpha_wino = None, None
                assert lib.yv3_conv2d_form(ctypes.byref(c)) == 0
                bound, key, other = (pb.WINO_X + pb.DIRECT_X) * t32u, "Winograd vs direct", "as direct tiles"
            y = relaunch_desc(c, n, "%s %s" % (what, other), dt, planes)
            e = (y.reshape(planes, -1).double().sum(0) - out.reshape(planes, -1).double().sum(0)).abs().reshape(-1, d.cout) / u
            worst = float(e.max())
            second[key] = max(second[key], worst / bound)
            if worst > bound:
                fails.append("%s: %.3g units from the launch %s at element %d (bound %.3g)" % (what, worst, other, int(e.argmax()), bound))
            del u, e
        else:
            c.options |= FORCED
            c.workspace, c.workspace_bytes = None, 0
            equal_bits(relaunch_desc(c, n, what + ", forced tile code 2", dt, planes), out, what + " vs forced tile code 2")
        del ins
        assert int(plan.flags.item()) == 0, "%s: status word %d" % (what, int(plan.flags.item()))

    # ---- the detections are yv3_decode of the heads' logits; nothing left behind
    torch.cuda.synchronize()
    assert torch.equal(again, dets), "%s: detections differ from yv3_decode of the heads' logits in %d elements" % (label, int((again != dets).sum()))
    assert int(plan.flags.item()) == 0, "%s: status word %d" % (label, int(plan.flags.item()))
    if plan.workspace is not None:
        assert not bool(plan.workspace[-SK_FLAG_BYTES:].any()), "%s: a stream-K hand-over flag was left set" % label

    by_cls = {}
    for cls, name, a, b, c3 in table:
        w = by_cls.setdefault(cls, [0.0, 0.0, 0.0, None])
        w[1], w[2] = max(w[1], b), max(w[2], c3)
        if a >= w[0]:
            w[0], w[3] = a, name
    secs = time.time() - t0
    print("plan %s: %d launches checked (%d stream-K, %d Winograd), %d failures; %.1f s" % (label, n_checked, n_sk, n_wino, len(fails), secs))
    head_line = "worst |got - ref| / eps | share of got != bf16(ref)" if mode == BF16 else "worst error in units | / torch fp32's | / the 2e-5 bar"
    print("    per class, %s: " % head_line + "; ".join(
        ("%s %.3g | %.2g (%s)" % (k, v[0], v[1], v[3])) if mode == BF16 else ("%s %.2f | %.2f | %.3f (%s)" % (k, v[0], v[1], v[2], v[3]))
        for k, v in sorted(by_cls.items())))
    print("    second path, full tensor, worst error / its bound: " + "; ".join("%s %.3f" % kv for kv in second.items()))
    return fails


@pytest.fixture(scope="module")
def sw1(sw1_stream):
    net = load_sw1_net(sw1_stream)
    params = pr.fold_params(net)
    return net.cuda(), params, pr.network_graph()


def _forward_and_check(net, params, graph, mode, x, label, table, key, which="all"):
    t0 = time.time()
    eng = net.engine(mode)
    with torch.no_grad():
        dets, plan = eng.forward(x)
    assert plan.B == x.shape[0] and eng.dtype == mode
    kernels = _assert_plan_is_the_tables(plan, table, key, label)
    fails = _check_plan(eng, plan, x, dets, params, graph, label, kernels, which)
    print("plan %s: forward + checks %.1f s wall" % (label, time.time() - t0))
    assert not fails, "\n".join(fails)
    return plan, kernels


def test_f32h2_one_image_plan_launch_by_launch(sw1, select_table):
    """a. F32H2 416x416 bs=1, all 75: stream-K at 1, 2, 4 and 8 channel tiles, the plain ping-pong 1x1 tiles, 128x64 and 128x32, the fused
    front, fused res64 and fused decode."""
    net, params, graph = sw1
    plan, kernels = _forward_and_check(net, params, graph, F32H2, torch.from_numpy(synth.images(1, 416, 2001)).cuda(), "a F32H2 416x416 bs=1",
                                       select_table, "f32h2/416/1")
    assert plan.workspace is not None and {k.split()[1] for k in kernels if " sk" in k} == {"nt=1", "nt=2", "nt=4", "nt=8"}


def test_f32h2_non_square_plan_launch_by_launch(sw1_stream, select_table):
    """b. F32H2 160 (H) x 224 (W) bs=3, all 75: pictures of 5x7 ... 40x56 cells -- odd sides, M tails, launches smaller than one tile."""
    net = YoloNet((224, 160)).eval()
    assert WeightManager(net).load_stream(sw1_stream) == sw1_stream.size
    params = pr.fold_params(net)
    x = torch.from_numpy(synth.images(3, 224, 2002)[:, :, :160, :224].copy()).cuda()
    plan, kernels = _forward_and_check(net.cuda(), params, pr.network_graph(), F32H2, x, "b F32H2 160x224 bs=3", select_table, None)
    assert plan.workspace is not None and any(" sk" in k for k in kernels)


def test_f32h2_one_lane_of_16_distinct_layers(sw1, select_table):
    """c. F32H2 416x416 bs=16 on one lane, the first launch of each distinct layer: W4_192x128 at 1, 2 and 4 tiles, 128x128_W4,
    128x128_W8 nt=8, no stream-K."""
    net, params, graph = sw1
    plan, kernels = _forward_and_check(net, params, graph, F32H2, torch.from_numpy(synth.images(16, 416, 2003)).cuda(), "c F32H2 416x416 bs=16",
                                       select_table, "f32h2/416/16", "distinct")
    assert plan.workspace is None and not any(" sk" in k for k in kernels)


def test_f32h2_two_lanes_of_16_distinct_layers(sw1, select_table):
    """d. Detector(net, 32, 416, 416, lanes=2), two concurrent lanes of 16.  Lane 0: distinct layers; lane 1: its Winograd launches and the
    three heads -- Winograd F(2x2) WINO_PINGPONG nt=4, 256x128_W8 at 1, 2 and 4 tiles; the shared status word and the scratch under
    concurrency."""
    net, params, graph = sw1
    t0 = time.time()
    x = torch.from_numpy(synth.images(32, 416, 2004)).cuda()
    det = Detector(net, 32, 416, 416, 0.5, 0.4, dtype=F32H2, lanes=2)
    assert det.lanes == 2
    with torch.no_grad():
        det(x)
    torch.cuda.synchronize()
    fails = []
    for i, (p, off) in enumerate(zip(det.lane_plans, det.lane_off)):
        assert p.B == 16 and p.workspace is None
        label = "d F32H2 416x416 lane %d of 2 x 16" % i
        kernels = _assert_plan_is_the_tables(p, select_table, "f32h2.two_lanes/416/16", label)
        assert sum(f == 1 for _, f in p.forms()) > 0
        fails += _check_plan(det.engine, p, x[off:off + 16], det.dets[off:off + 16], params, graph, label, kernels, "distinct" if i == 0 else "wino")
    assert bool(torch.isfinite(det.dets).all())
    print("plan d: detector + checks of both lanes %.1f s wall" % (time.time() - t0))
    assert not fails, "\n".join(fails)


def test_f32x3_plan_of_4_distinct_layers(sw1, select_table):
    """e. F32X3 416x416 bs=4, distinct layers: 256x128_W8 plain, 128x128_W8 plain at 1 to 8 tiles, yv3_conv0 with a three-plane output."""
    net, params, graph = sw1
    plan, _ = _forward_and_check(net, params, graph, F32X3, torch.from_numpy(synth.images(4, 416, 2005)).cuda(), "e F32X3 416x416 bs=4",
                                 select_table, "f32x3/416/4", "distinct")
    assert not plan.fused_front and plan.conv0_out.shape[0] == 3


def test_bf16_one_image_plan_launch_by_launch(sw1, select_table):
    """f. BF16 416x416 bs=1, all 75, held to the BF16 bar (conv_ref: criteria A and B, bf16-rounded weights); heads to the fp32 bar."""
    net, params, graph = sw1
    _forward_and_check(net, params, graph, BF16, torch.from_numpy(synth.images(1, 416, 2006)).cuda(), "f BF16 416x416 bs=1", select_table, "bf16/416/1")
