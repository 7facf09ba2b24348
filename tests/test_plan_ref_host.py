"""tests/plan_ref.py against the oracle, on the CPU: a mistake in the float64 reference of the plan tests (tests/test_gpu_plan_local.py)
must not pass for a kernel bug, or hide one."""
import torch

from oracle import oracle_cpu as oc
from yolo_v3_amd import synth
from tests import conv_ref as cr
from tests import plan_ref as pr
from tests.helpers import load_sw1_net

# max |oracle fp32 tap - float64 chain| / max(1, |chain|) over the 75 taps of the 64x64 B=2 case below: observed 7.3e-6, at
# pre_det1.mlist.0 (the fp32 oracle's own round-off, compounded through 53 layers -- the looser side; one torch-fp32 layer on float64-exact
# inputs is up to 6.9e-6 away, at the K = 4608 pre_det1.mlist.1); asserted 4x that.  A wiring, BatchNorm or residual-order mistake is O(1).
ORACLE_ROUNDOFF = 7.3e-6


def test_float64_chain_reproduces_the_oracle_taps(sw1_stream):
    """plan_ref.chain -- network_graph wiring (routes, upsample + concat order, residual after the activation), fold_params (BatchNorm folded
    in float64 from the modules) and conv_desc_ref, each layer fed the chain's own float64 output -- reproduces all 75 taps of
    oracle_cpu.head_logits on a 64x64 B=2 input with SW-1 weights within fp32 round-off of the oracle (4 x the observed 7.3e-6);
    the sampled-rows path, the fused-pair path and the torch-fp32 yardstick agree with the full path on the same inputs."""
    net = load_sw1_net(sw1_stream)
    sd = oc.state_dict_from_stream(sw1_stream)[0]
    x = torch.from_numpy(synth.images(2, 64, 31))
    taps = []
    with torch.no_grad():
        oc.head_logits(sd, x, taps)
    graph = pr.network_graph()
    assert [n.name for n in graph] == [name for name, _ in taps]
    params = pr.fold_params(net)
    acts = pr.chain(params, x, graph)
    worst, where = 0.0, None
    for name, t in taps:
        ref = acts[name]
        got = t.permute(0, 2, 3, 1)
        assert tuple(got.shape) == tuple(ref.shape), name
        e = float(pr.norm_err(got, ref).max())
        if e > worst:
            worst, where = e, name
    print("float64 chain vs the fp32 oracle's 75 taps: worst %.3g at %s (bound %.3g)" % (worst, where, 4 * ORACLE_ROUNDOFF))
    assert worst <= 4 * ORACLE_ROUNDOFF, (worst, where)

    # the sampled-rows path == the full path, on every kind of node (3x3 s1 + residual, 3x3 s2, upsample + concat, head)
    by_name = {n.name: n for n in graph}
    full = dict(acts)
    full[pr.IMAGE] = x.double().permute(0, 2, 3, 1)
    for name in ("feature.mlist.0", "feature.mlist.1", "feature.mlist.2.conv2", "feature.mlist.15", "pre_det2.mlist.0", "pre_det3.mlist.0",
                 "pre_det1.mlist.1", "pre_det3.mlist.6"):
        n = by_name[name]
        B, Ho, Wo, C = acts[name].shape
        rows = cr.sample_rows(B, Ho, Wo, seed=5, n_random=64, last=16)
        got = pr.launch_ref(n, params[name], full[n.x], full.get(n.x2), full.get(n.residual), pixels=rows)
        assert float((got - acts[name].reshape(-1, C)[rows]).abs().max()) <= 1e-12, name
        # ... and the reference's own fp32 arithmetic on the same inputs is fp32-close to it
        f32 = pr.torch_f32_rows(n, params[name], full[n.x], full.get(n.x2), full.get(n.residual), pixels=rows)
        assert float(pr.norm_err(f32, got).max()) <= 4 * ORACLE_ROUNDOFF, name
    # the fused pairs (intermediate never materialised)
    for a, b, src in (("feature.mlist.0", "feature.mlist.1", pr.IMAGE), ("feature.mlist.2.conv1", "feature.mlist.2.conv2", "feature.mlist.1")):
        B, Ho, Wo, C = acts[b].shape
        rows = cr.sample_rows(B, Ho, Wo, seed=6, n_random=64, last=16)
        res = full[by_name[b].residual] if by_name[b].residual else None
        got = pr.fused_pair_ref(by_name[a], params[a], by_name[b], params[b], full[src], rows, residual=res, chunk=1)
        assert float((got - acts[b].reshape(-1, C)[rows]).abs().max()) <= 1e-12, b
