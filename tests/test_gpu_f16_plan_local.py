"""Every launch of the F16 plan at 416x416 bs=1 -- all 75 convolutions, as tests/test_gpu_plane_plan_local.py's case f does for BF16 --
against float64 on the tensors the GPU itself fed each launch (-m gpu, through the C-ABI):

  * wiring: the descriptor's input pointers name the producers plan_ref.network_graph expects, and the plan is the BF16 plan's, kernel
    line for kernel line (the selection of an F16 descriptor is the BF16 descriptor's);
  * value: the F16 bar (tests/conv_ref_f16.py, criteria A and B) on plan_ref.rows_of, with the weights as the definition rounds them --
    each output channel scaled to max|w| in [1, 2) by a power of two, rounded to fp16, the inverse in alpha -- and the heads' fp32
    logits at conv_ref.F32_BAR (2e-5);
  * the fused front and first residual block: their un-fused launches of the plan's own descriptors, each within the bar, equal the fused
    kernels' outputs bit for bit;
  * independent path: every launch relaunched with forced tile code 8 into a NaN-filled buffer with a NaN canary behind it (every
    element written, canary intact): bit-identical;
  * the fused-decode heads: relaunched with dec_out = NULL, yv3_decode of their logits == the plan's detections, bit for bit;
  * status word 0 throughout."""
import ctypes
import time

import pytest
import torch

from yolo_v3_amd import _ffi, engine, synth
from tests import conv_ref as cr, conv_ref_f16 as cf, f16_ref
from tests import plan_ref as pr
from tests.helpers import load_sw1_net, desc_inputs_by_pointer, copy_desc, relaunch_desc

pytestmark = pytest.mark.gpu

F16, BF16, F32 = _ffi.F16, _ffi.BF16, _ffi.F32
NAN = float("nan")
FORCED = _ffi.TILE_256x256_ROLL << _ffi.OPT_TILE_SHIFT          # code 8


def _f16_params(params):
    """plan_ref.fold_params as the F16 definition rounds them: w -> f16(w 2^e) per output channel, alpha -> alpha 2^-e (1 for a head)."""
    out = {}
    for name, p in params.items():
        if p.w.shape[1] == 3:
            out[name] = p
            continue
        wq, inv = f16_ref.round_weight(p.w)
        out[name] = p._replace(w=wq, alpha=(p.alpha if p.alpha is not None else torch.ones(p.w.shape[0], dtype=torch.float64)) * inv.double())
    return out


def test_f16_one_image_plan_launch_by_launch(sw1_stream):
    t0 = time.time()
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    net = load_sw1_net(sw1_stream)
    params, graph = _f16_params(pr.fold_params(net)), pr.network_graph()
    net = net.cuda()
    x = torch.from_numpy(synth.images(1, 416, 2006)).cuda()
    lib, eng = _ffi.lib(), net.engine(F16)
    with torch.no_grad():
        dets, plan = eng.forward(x)
        eb = net.engine(BF16)
        eb.ensure_packed()
        ref_kernels = eb.plan(1, 416, 416).kernels()
    assert eng.dtype == F16 and plan.B == 1 and plan.fused_decode and len(plan.head_descs) == 3
    assert plan.fused_front and plan.fused_res64 and plan.first_desc == 3 and plan.workspace is None and plan.wino_ws is None
    kernels = plan.kernels()
    assert kernels == ref_kernels and plan.launches() == [1] * len(kernels) and all(f == 0 for _, f in plan.forms())
    print("plan F16 416x416 bs=1 reaches: %s" % "; ".join(sorted(set(kernels))))
    torch.cuda.synchronize()
    assert int(plan.flags.item()) == 0
    names = desc_inputs_by_pointer(plan)
    by_name = {n.name: n for n in graph}
    B, H, W = 1, 416, 416
    img = x.cpu().permute(0, 2, 3, 1).contiguous()
    fails, worst = [], {}

    def host(name):
        if name is None:
            return None
        return img if name == pr.IMAGE else engine.from_planes(plan.layer_out[name], F16).cpu()

    def value(out, node, ins, rows, cls, what):
        p, C = params[node.name], node.spec.cout
        flat = out.reshape(-1, C)
        assert bool(torch.isfinite(flat).all()), "%s: non-finite output" % what
        got = flat[rows.cuda()].double().cpu()
        ref = pr.launch_ref(node, p, *ins, pixels=rows)
        if out.dtype == torch.float32:
            e = float(pr.norm_err(got, ref).max())
            worst[cls] = max(worst.get(cls, (0.0, 0.0)), (e / cf.F32_BAR, 0.0))
            if e > cf.F32_BAR:
                fails.append("%s: fp32 logits %.3g x the 2e-5 bar from float64" % (what, e / cf.F32_BAR))
            return
        mag = cr.conv_desc_mag(ins[0], p.w, p.beta, p.alpha, ins[2], ins[1], node.cin_up, node.spec.stride, pixels=rows)
        r = cf.f16_report(got, ref, mag, node.spec.k ** 2 * node.spec.cin)
        worst[cls] = max(worst.get(cls, (0.0, 0.0)), (r["worst"], r["share"]))
        if not (r["a_ok"] and r["b_ok"]):
            fails.append("%s: F16 bar: %d elements outside their interval (first %s), share of got != f16(ref) %.3g (cap %.1g)" % (
                what, r["outside"], r["first"], r["share"], cf.F16_SHARE_CAP))

    def equal_bits(a, b, what):
        if not torch.equal(a.reshape(-1), b.reshape(-1)):
            fails.append("%s: %d elements differ" % (what, int((a.reshape(-1) != b.reshape(-1)).sum())))

    # ---- the front: yv3_conv0 alone, then the un-fused launches of the plan's own descriptors against the fused kernels
    g0, g1, g2, g3 = graph[:4]
    assert [names(plan.descs[j]) for j in range(3)] == [(g.x, g.x2, g.residual) for g in (g1, g2, g3)]
    eng.run_conv0(plan, x)
    value(plan.conv0_out, g0, (img, None, None), pr.rows_of(B, H, W, seed=100), "conv0", "yv3_conv0 %s" % g0.name)
    h1, w1 = H // 2, W // 2
    n1 = B * h1 * w1 * 64
    m0 = host(g0.name)
    y1 = relaunch_desc(copy_desc(plan.descs[0]), n1, "un-fused %s" % g1.name, torch.float16, 1)
    value(y1, g1, (m0, None, None), pr.rows_of(B, h1, w1, seed=101), "un-fused front", "un-fused %s" % g1.name)
    equal_bits(y1, plan.layer_out[g1.name], "fused front vs the two-launch path")
    m1 = host(g1.name)
    _ffi.check(lib.yv3_conv2d(ctypes.byref(plan.descs[1]), _ffi.stream_ptr()), "un-fused " + g2.name)
    value(plan.layer_out[g2.name], g2, (m1, None, None), pr.rows_of(B, h1, w1, seed=102), "un-fused res64", "un-fused %s" % g2.name)
    y3 = relaunch_desc(copy_desc(plan.descs[2]), n1, "un-fused %s" % g3.name, torch.float16, 1)
    value(y3, g3, (host(g2.name), None, m1), pr.rows_of(B, h1, w1, seed=103), "un-fused res64", "un-fused %s" % g3.name)
    equal_bits(y3, plan.layer_out[g3.name], "fused res64 vs the two-launch path")
    del y1, y3, m0, m1

    # ---- the launches of the sequence
    forms = plan.forms()
    heads = {di: k for k, (di, _, _) in enumerate(plan.head_descs)}
    again = torch.full_like(dets, NAN)
    for i, j in enumerate(range(plan.first_desc, plan.n_desc)):
        d = plan.descs[j]
        name = eng.specs[forms[i][0]].name
        node = by_name[name]
        assert names(d) == (node.x, node.x2, node.residual) and d.cin_up == node.cin_up, (name, names(d))
        assert d.dtype == F16 and d.B == B
        head = j in heads
        ho, wo = cr.out_hw(d.H, d.W, d.k, d.stride)
        n = B * ho * wo * d.cout
        cls = ("head " if head else "") + kernels[i].split()[0]
        what = "launch %d %s [%s]" % (j, name, kernels[i])
        rows = pr.rows_of(B, ho, wo, seed=j)
        ins = (host(node.x), host(node.x2), host(node.residual))
        c = copy_desc(d)
        if head:
            assert d.y is None and d.dec_out and d.out_dtype == F32
            c.dec_out = None
            out = relaunch_desc(c, n, what + ", dec_out = NULL")
            value(out, node, ins, rows, cls, what)
            anc, stride, row0, _, hh, ww = plan.decode_args[heads[j]]
            _ffi.check(lib.yv3_decode(out.data_ptr(), d.cout, anc, stride, again.data_ptr() + row0 * plan.attrib * 4, plan.N * plan.attrib,
                                      B, hh, ww, eng.num_class, _ffi.stream_ptr()), "yv3_decode")
            c, dt = copy_desc(c), torch.float32
        else:
            out = plan.layer_out[name]
            assert out.numel() == n and out.data_ptr() == d.y and d.out_dtype == F16
            value(out, node, ins, rows, cls, what)
            dt = torch.float16
        c.options |= FORCED
        equal_bits(relaunch_desc(c, n, what + ", forced tile code 8", dt, 1), out, what + " vs forced tile code 8")
        assert int(plan.flags.item()) == 0, "%s: status word %d" % (what, int(plan.flags.item()))

    torch.cuda.synchronize()
    assert torch.equal(again, dets), "detections differ from yv3_decode of the heads' logits in %d elements" % int((again != dets).sum())
    assert int(plan.flags.item()) == 0
    print("plan F16 416x416 bs=1: 75 launches checked, %d failures; %.1f s" % (len(fails), time.time() - t0))
    print("    per class, worst |got - ref| / eps | share of got != f16(ref) (heads: error / 2e-5): " + "; ".join(
        "%s %.3g | %.2g" % (k, v[0], v[1]) for k, v in sorted(worst.items())))
    assert not fails, "\n".join(fails)
