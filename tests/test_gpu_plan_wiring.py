"""The descriptors of an inference plan against tests/plan_ref.network_graph, for every kind of plan the engine builds (-m gpu): nothing is
launched beyond the weight packing.  B = 2, 64 (H) x 96 (W) -- non-square, grids 2x3, 4x6 and 8x12 -- SW-1 weights.

Cases: the six math modes (I8 with every scale 1.0), each as the inference plan, as the ``logits=True`` plan and as one of two lanes;
prefix engines of 4, 8, 52 and 68 convolutions in F32 and BF16.  For every descriptor, mapped through ``desc_spec`` to its plan_ref.Node:

  * x / x2 / residual are the ``layer_out`` buffers of the node's producers, y the node's own (I8: convolution 4 reads ``front_q``, the
    quantised front; a head that decodes in its epilogue has no y and no ``layer_out`` entry);
  * B, H, W (the node's input picture, worked out here from the graph: a join reads at its route's size), cin, cin_up, cout, k, stride,
    act, and the launch and output formats the mode implies;
  * one descriptor per convolution behind feature.mlist.0, ``first_desc`` by the mode's fused front, ``head_descs`` / ``logits`` / ``rows``
    / ``decode_args`` by the mode and the prefix length.
"""
import pytest
import torch

from yolo_v3_amd import _ffi, arch, engine
from tests import conv_ref as cr
from tests import plan_ref as pr
from tests.helpers import load_sw1_net

pytestmark = pytest.mark.gpu

F32, BF16, F32X3, F32H2, F16, I8 = _ffi.F32, _ffi.BF16, _ffi.F32X3, _ffi.F32H2, _ffi.F16, _ffi.I8
MODES = {"F32": F32, "BF16": BF16, "F32X3": F32X3, "F32H2": F32H2, "F16": F16, "I8": I8}
B, H, W = 2, 64, 96
GRIDS = [(2, 3), (4, 6), (8, 12)]
HEADS = [58, 66, 74]                 # the three plain head convs, in conv_specs order


@pytest.fixture(scope="module")
def net(sw1_stream):
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    n = load_sw1_net(sw1_stream).cuda()
    n.int8_scales = {name: 1.0 for name in engine.int8_scale_names(arch.conv_specs(80))}
    return n


@pytest.fixture(scope="module")
def graph():
    """(nodes, {name: (h, w) the node reads}) at H x W."""
    nodes = pr.network_graph()
    out, reads = {pr.IMAGE: (H, W)}, {}
    for n in nodes:
        reads[n.name] = out[n.x2 if n.x2 is not None else n.x]
        out[n.name] = cr.out_hw(*reads[n.name], n.spec.k, n.spec.stride)
    return nodes, reads


def _check(eng, plan, graph, mode, logits, two_lanes):
    nodes, reads = graph
    n_conv, i8 = eng.n_conv, mode == I8
    prefix = n_conv < 75
    out_ptr = {name: t.data_ptr() for name, t in plan.layer_out.items()}
    fused_decode = mode != F32 and not logits and not prefix
    assert plan.fused_decode == fused_decode
    assert plan.first_desc == (0 if mode == F32X3 else 3) and plan.fused_front == (mode != F32X3) and plan.fused_res64 == (mode != F32X3)
    assert plan.n_desc == len(plan.descs) == n_conv - 1 and plan.desc_spec == list(range(1, n_conv))
    heads = [i for i in HEADS if i < n_conv]
    assert plan.head_descs == ([] if mode == F32 else [(i - 1,) + GRIDS[HEADS.index(i)] for i in heads])
    assert set(out_ptr) == {nodes[i].name for i in range(n_conv) if not (fused_decode and i in HEADS)}
    assert len(set(out_ptr.values())) == len(out_ptr) and plan.conv0_out is plan.layer_out[nodes[0].name]
    assert (plan.front_q is not None) == i8 and (plan.front_inv_s == 1.0 if i8 else plan.front_inv_s == 0.0)

    def ptr(name, j):
        if name is None:
            return None
        return plan.front_q.data_ptr() if (i8 and j == engine.I8_FIRST) else out_ptr[name]

    for di in range(plan.n_desc):
        d, j = plan.descs[di], plan.desc_spec[di]
        node = nodes[j]
        sp, what = node.spec, "%s (descriptor %d)" % (node.name, di)
        assert (d.x, d.x2, d.residual) == (ptr(node.x, j), out_ptr.get(node.x2), out_ptr.get(node.residual)), what
        assert (node.x2 is None or node.x2 in out_ptr) and (node.residual is None or node.residual in out_ptr), what
        assert d.y == out_ptr.get(node.name) and (d.y is None) == (fused_decode and j in HEADS), what
        assert (d.B, d.H, d.W) == (B,) + reads[node.name], what
        assert (d.cin, d.cin_up, d.cout, d.k, d.stride) == (sp.cin, node.cin_up, sp.cout, sp.k, sp.stride), what
        assert d.act == (_ffi.ACT_LEAKY if sp.bn else _ffi.ACT_LINEAR), what
        launch = (I8 if (j >= engine.I8_FIRST and sp.bn) else BF16) if i8 else mode
        feeds_head = j + 1 in HEADS
        assert d.dtype == launch and d.out_dtype == (F32 if j in HEADS else BF16 if (i8 and feeds_head) else launch), what
        assert bool(d.options & _ffi.OPT_TWO_LANES) == two_lanes and d.flags == plan.flags.data_ptr(), what
    assert (plan.workspace is not None) == (mode == F32H2 and not two_lanes)
    assert (plan.wino_ws is not None) == (mode in (F32H2, F32))

    # the heads: logits, rows, decode parameters
    assert [(h, w) for _, h, w in plan.logits] == GRIDS and plan.rows == [18, 72, 288] and plan.N == 378 and plan.attrib == 85
    for (lg, h, w), i in zip(plan.logits, HEADS):
        if i >= n_conv or fused_decode:
            assert lg is None
        else:
            assert lg is plan.layer_out[nodes[i].name] and tuple(lg.shape) == (B, h, w, 255) and lg.dtype == torch.float32
    if prefix:
        assert plan.decode_args == []
    else:
        assert [(a[1], a[2], a[4], a[5]) for a in plan.decode_args] == [(32.0, 0, 2, 3), (16.0, 18, 4, 6), (8.0, 90, 8, 12)]
        assert all(a[3] is lg for a, (lg, _, _) in zip(plan.decode_args, plan.logits))


@pytest.mark.parametrize("variant", ["plain", "logits", "two_lanes"])
@pytest.mark.parametrize("mode", list(MODES))
def test_descriptors_follow_the_graph(net, graph, mode, variant):
    eng = net.engine(MODES[mode])
    eng.ensure_packed()
    logits, two_lanes = variant == "logits", variant == "two_lanes"
    with torch.cuda.device(eng.device):
        plan = engine.Plan(eng, B, H, W, two_lanes=two_lanes, logits=logits)
    _check(eng, plan, graph, MODES[mode], logits, two_lanes)


@pytest.mark.parametrize("n_conv", [4, 8, 52, 68])
@pytest.mark.parametrize("mode", ["F32", "BF16"])
def test_prefix_plan_descriptors_follow_the_graph(net, graph, mode, n_conv):
    eng = net.prefix_engine(MODES[mode], n_conv)
    eng.ensure_packed()
    assert len(eng.packed) == n_conv
    with torch.cuda.device(eng.device):
        plan = engine.Plan(eng, B, H, W)
    _check(eng, plan, graph, MODES[mode], True, False)
