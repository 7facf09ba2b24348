"""tests/plane_bar.py on the CPU: the bar that tests/test_gpu_plane_plan_local.py holds every plane-mode launch to accepts a correct
fp16-plane launch and rejects the faults the fixed 2e-5 bar cannot see -- decided here, before any GPU figure exists."""
import time

import torch

from yolo_v3_amd import synth
from tests import conv_ref as cr
from tests import plan_ref as pr
from tests import plane_bar as pb
from tests.helpers import load_sw1_net


def test_bar_accepts_the_emulated_plan_and_rejects_every_fault(sw1_stream):
    """SW-1 weights, 160x160, B = 2, all 75 launches, each fed the (correct) emulated network's own outputs, judged like a GPU launch:
    float64 and torch fp32 on plan_ref.rows_of of the tensors the launch read.  The correct emulation passes bars 1 to 3 on 75 / 75; each
    of the five faults fails bar 2 on EVERY launch it applies to (dropped w_lo x_hi / w_hi x_lo: 74, the first layer's operands apart;
    output hi plane only: 72; residual hi only: 23; LeakyReLU slope held in fp16: 72); a truncating hi fails check 3 on about half the
    elements of every stored tensor while bars 1 and 2 still pass it."""
    t0 = time.time()
    net = load_sw1_net(sw1_stream)
    params, graph = pr.fold_params(net), pr.network_graph()
    B, S = 2, 160
    acts = {pr.IMAGE: pb.split_h2(torch.from_numpy(synth.images(B, S, 77)).permute(0, 2, 3, 1).contiguous())}
    torch_u, bar2, share = [], [], []
    mildest = {f: (float("inf"), None, 0, 0) for f in pb.FAULTS}            # fault -> (error / bar 2 at its mildest launch, name, rejected, applicable)
    trunc_share = []
    with torch.no_grad():
        for j, node in enumerate(graph):
            p = params[node.name]
            ins = [acts.get(node.x), acts.get(node.x2), acts.get(node.residual)]
            faults = [f for f in pb.FAULTS if pb.fault_applies(f, node, p)]
            out = pb.emulate_h2(node, p, *ins, faults=faults)
            acts[node.name] = out[None]
            x, x2, res = (pb.merge(t) if t is not None else None for t in ins)
            Bx, H, W = (x2 if node.cin_up else x).shape[:3]
            ho, wo = cr.out_hw(H, W, node.spec.k, node.spec.stride)
            rows = pr.rows_of(Bx, ho, wo, seed=j)
            ref = pr.launch_ref(node, p, x, x2, res, pixels=rows)
            mag = cr.conv_desc_mag(x, p.w, p.beta, p.alpha, res, x2, node.cin_up, node.spec.stride, pixels=rows)
            t32 = pr.torch_f32_rows(node, p, x, x2, res, pixels=rows)
            K, planes = node.spec.k ** 2 * node.spec.cin, p.alpha is not None

            def verdict(o):
                return pb.judge(pb.merge(o).reshape(-1, node.spec.cout)[rows], ref, mag, t32, K, fp16_planes=planes)
            v = verdict(out[None])
            assert v.ok1 and v.ok2, "correct emulation, launch %d %s: %.3g units (bar 1 %.3g, bar 2 %.3g, torch fp32 %.3g)" % (
                j, node.name, v.units, v.bar1, v.bar2, v.torch)
            torch_u.append(v.torch), bar2.append(v.bar2), share.append(v.units / v.bar2)
            if planes:
                hi, lo = out[None]
                assert pb.split_violations(torch.stack((hi.half(), lo.half()))) == 0, node.name
                th, tl = pb.trunc_split_h2(pb.merge(out[None]))                 # (re-splitting hi + lo: the same values, a truncated hi)
                bad = pb.split_violations(torch.stack((th.half(), tl.half())))
                trunc_share.append(bad / th.numel())
                tv = verdict((th, tl))
                assert tv.ok1 and tv.ok2, node.name                             # ... which the value bars cannot see
            for f in faults:
                fv = verdict(out[f])
                m, name, n_rej, n_app = mildest[f]
                r = fv.units / fv.bar2
                mildest[f] = (min(m, r), node.name if r < m else name, n_rej + (not fv.ok2), n_app + 1)
                assert not fv.ok2, "fault %s passes bar 2 at launch %d %s: %.3g units, bar %.3g" % (f, j, node.name, fv.units, fv.bar2)
    print("emulated F32H2 plan, %dx%d B=%d, 75 launches: torch fp32 %.1f - %.1f units; bar 2 %.1f - %.1f units; correct emulation %.2f - %.2f of bar 2; "
          "truncating hi: check 3 fails on %.2f - %.2f of the elements; %.0f s" % (S, S, B, min(torch_u), max(torch_u), min(bar2), max(bar2), min(share), max(share),
                                                                                    min(trunc_share), max(trunc_share), time.time() - t0))
    for f in pb.FAULTS:
        m, name, n_rej, n_app = mildest[f]
        print("    fault %-13s mildest %.1f x bar 2 (%s), over the bar on %d / %d launches" % (f, m, name, n_rej, n_app))
    assert [mildest[f][3] for f in pb.FAULTS] == [74, 74, 72, 23, 72]
    assert min(trunc_share) > 0.25


def test_split_check_is_exact_on_every_bit_pattern():
    """check 3 on every finite fp16 / bf16 value as the upper plane: half_ulp equals 2^(binade - mantissa bits - 1) (frexp, subnormals at the
    smallest normal's spacing); a lower plane of exactly half an ulp -- what a nearest split leaves at a tie -- passes, one of a whole ulp fails."""
    for dtype, top in ((torch.float16, 0x7BFF), (torch.bfloat16, 0x7F7F)):
        mant, emin = pb._FORMAT[dtype]
        up = torch.arange(0, top + 1, dtype=torch.int32).to(torch.int16).view(dtype)
        up = torch.cat((up, -up))
        hu = pb.half_ulp(up)
        m, e = torch.frexp(up.double().abs())
        binade = torch.where(m > 0, e - 1, torch.full_like(e, emin)).clamp(min=emin)
        assert torch.equal(hu, torch.ldexp(torch.ones_like(hu), binade - mant - 1)), dtype
        assert pb.split_violations(torch.stack((up, hu.to(dtype)))) == 0, dtype
        assert pb.split_violations(torch.stack((up, -hu.to(dtype)))) == 0, dtype
        assert pb.split_violations(torch.stack((up, (2 * hu).to(dtype)))) == up.numel(), dtype
