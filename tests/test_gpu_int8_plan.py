"""The I8 plan end to end on the GPU (SW-1 weights, 64 x 64, B = 2, calibrated on the same batch): starting from the GPU's own front
output, all 68 int8 layers replayed in numpy (tests/int8_ref.py, chained, wired by arch.conv_specs and the architecture's routes -- not
by the plan's descriptors) equal every int8 ``layer_out`` buffer and the three head inputs bit for bit; the front and head launches
equal the same launches of a BF16 engine; detect() runs under graph capture and repeats itself; a changed scale re-packs.

A second fixture runs the same replay at 64 x 96 (height != width) with B = 3, calibrated on its own batch: exchanged H and W in the plan's
buffers or in the upsample + concat descriptors cannot pass it, and its two lanes take 2 and 1 images."""
import time

import numpy as np
import pytest
import torch

from yolo_v3_amd import _ffi, arch, engine, synth, detect, Detector, YoloNet, WeightManager
from tests import int8_ref as ir
from tests.helpers import relaunch_desc

pytestmark = pytest.mark.gpu

I8, BF16, F32 = _ffi.I8, _ffi.BF16, _ffi.F32
SIZE, B = 64, 2
RECT_H, RECT_W, RECT_B = 64, 96, 3


def _run(H, W, nb, seed):
    """One calibrated network, its I8 logits plan after one forward, and the numpy replay of the 68 int8 layers -- shared, read-only."""
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    net = YoloNet((H, W), numClass=80).eval()
    stream = synth.weight_stream(80)
    assert WeightManager(net).load_stream(stream) == stream.size
    net = net.cuda()
    x = torch.from_numpy(np.ascontiguousarray(synth.images(nb, max(H, W), seed)[:, :, :H, :W])).cuda()
    assert tuple(x.shape) == (nb, 3, H, W)
    scales = net.calibrate_int8([x])
    net.math_mode = I8
    specs = arch.conv_specs(80)
    eng = net.engine()
    assert eng.dtype == I8
    _, plan = eng.forward(x, logits=True)
    torch.cuda.synchronize()
    f32 = net.engine(F32)                       # packed by the calibration: the folded BatchNorm of every layer
    params = {i: (net.get_submodule(specs[i].name).conv.weight.detach().cpu().numpy(), f32.packed[i].alpha.cpu().numpy(), f32.packed[i].beta.cpu().numpy())
              for i in ir.int8_layers(specs)}
    front = plan.layer_out[specs[ir.I8_FIRST - 1].name]
    front_q = ir.quantize_act(front[0].float().cpu().numpy(), scales[specs[ir.I8_FIRST - 1].name])
    t0 = time.time()
    ref = ir.run_layers(specs, params, scales, front_q)
    print("i8 plan | %d x %d, B = %d: numpy replay of the 68 int8 layers %.2f s" % (H, W, nb, time.time() - t0))
    return dict(net=net, x=x, scales=dict(scales), specs=specs, eng=eng, plan=plan, ref=ref, front_q=front_q, H=H, W=W, B=nb)


@pytest.fixture(scope="module")
def run():
    return _run(SIZE, SIZE, B, 4242)


@pytest.fixture(scope="module")
def run_rect():
    """The same at 64 x 96 with an odd batch, calibrated on its own batch."""
    return _run(RECT_H, RECT_W, RECT_B, 4243)


def test_calibration_gives_69_positive_scales(run):
    names = ir.scale_names(run["specs"])
    assert len(names) == 69 and sorted(run["scales"]) == sorted(names)
    assert all(0 < v < float("inf") for v in run["scales"].values())
    lo, hi = min(run["scales"].values()), max(run["scales"].values())
    print("i8 plan | scales: min %.4g max %.4g" % (lo, hi))


def _front_is_the_bf16_engines_and_is_quantised_by_definition(run):
    net, x, specs, plan = run["net"], run["x"], run["specs"], run["plan"]
    _, pb = net.engine(BF16).forward(x, logits=True)
    torch.cuda.synchronize()
    name = specs[ir.I8_FIRST - 1].name
    assert plan.layer_out[name].dtype == torch.bfloat16
    assert torch.equal(plan.layer_out[name].view(torch.int16), pb.layer_out[name].view(torch.int16)), "the front launches differ from the BF16 engine's"
    got = plan.front_q[0].cpu().numpy()
    assert got.dtype == np.int8 and np.array_equal(got, run["front_q"]), "%d quantised front values differ" % int((got != run["front_q"]).sum())
    assert np.abs(got).max() == 127 and got.min() >= -127


def test_front_is_the_bf16_engines_and_is_quantised_by_definition(run):
    _front_is_the_bf16_engines_and_is_quantised_by_definition(run)


def _all_int8_layers_bit_identical_to_the_numpy_replay(run):
    """Every int8 layer_out buffer (int8, or for the three layers in front of a head the same integers as bf16 = the head's input)."""
    specs, plan, ref = run["specs"], run["plan"], run["ref"]
    layers = ir.int8_layers(specs)
    assert len(layers) == 68
    head_inputs, spread = 0, []
    for i in layers:                                        # execution order: the first difference is the first wrong layer
        buf = plan.layer_out[specs[i].name]
        to_head = i + 1 < len(specs) and not specs[i + 1].bn
        assert buf.dtype == (torch.bfloat16 if to_head else torch.int8), specs[i].name
        head_inputs += to_head
        got = buf[0].float().cpu().numpy()
        want = ref[i].astype(np.float32)
        assert got.shape == want.shape and got.shape[0] == run["B"], (specs[i].name, got.shape, want.shape)
        nbad = int((got != want).sum())
        assert nbad == 0, "first differing layer: %s (conv %d): %d of %d values differ, max |d| %g" % (specs[i].name, i, nbad, want.size, np.abs(got - want).max())
        spread.append(len(np.unique(want)))
    assert head_inputs == 3
    print("i8 plan | %d x %d, B = %d | 68 layers bit-identical | distinct values per layer: min %d median %d" % (run["H"], run["W"], run["B"], min(spread), int(np.median(spread))))
    assert np.median(spread) > 50, "the activations do not use the int8 range: the replay checks little"


def test_all_int8_layers_bit_identical_to_the_numpy_replay(run):
    _all_int8_layers_bit_identical_to_the_numpy_replay(run)


def test_head_launches_equal_bf16_launches_with_folded_scale(run):
    """Each head conv of the I8 plan == a BF16 launch built here from the module's parameters: its input the bf16 integers, alpha = the
    input tensor's scale for every channel, bias as beta."""
    net, specs, plan, scales = run["net"], run["specs"], run["plan"], run["scales"]
    heads = [i for i, sp in enumerate(specs) if not sp.bn]
    assert len(heads) == 3
    for i, (lg, h, w) in zip(heads, plan.logits):
        mod = net.get_submodule(specs[i].name)
        pc = engine.pack_conv(mod, specs[i], BF16)
        assert pc.alpha is None
        pc.alpha = torch.full((specs[i].cout,), float(np.float32(scales[specs[i - 1].name])), device="cuda")
        xin = plan.layer_out[specs[i - 1].name]
        d = engine.make_desc(pc, xin, None, B, h, w, dtype=BF16, out_dtype=F32)
        got = relaunch_desc(d, B * h * w * specs[i].cout, specs[i].name)
        assert torch.equal(got.view(torch.int32), lg.reshape(-1).view(torch.int32)), "%s differs from the BF16 launch" % specs[i].name
        assert bool(torch.isfinite(lg).all())


def test_detect_runs_under_graph_capture_and_repeats(run):
    net, x = run["net"], run["x"]
    with torch.no_grad():
        eager = detect(net, x, obj_conf_thr=0.05)
        gdet = Detector(net, B, SIZE, SIZE, 0.05, 0.4, graph=True, lanes=1)
        first = gdet(x)
        dets1 = gdet.dets.clone()
        second = gdet(x)
    assert gdet.engine.dtype == I8 and torch.equal(dets1, gdet.dets) and bool(torch.isfinite(dets1).all())
    assert len(first) == len(second) == len(eager)
    for a, b_, c in zip(first, second, eager):
        assert torch.equal(a, b_) and torch.equal(a, c)
    print("i8 plan | boxes per image under graph replay: %s" % [int(t.shape[0]) if t.numel() else 0 for t in first])


def _two_lanes_equal_one_lane(run):
    net, x, nb, H, W = run["net"], run["x"], run["B"], run["H"], run["W"]
    with torch.no_grad():
        one = Detector(net, nb, H, W, 0.05, 0.4, lanes=1)
        r1 = one(x)
        two = Detector(net, nb, H, W, 0.05, 0.4, lanes=2)
        r2 = two(x)
    assert (one.lanes, two.lanes) == (1, 2) and two.engine.dtype == I8
    assert [p.B for p in two.lane_plans] == [nb - nb // 2, nb // 2]
    assert torch.equal(one.dets, two.dets)
    assert len(r1) == len(r2) == nb and all(torch.equal(a, b_) for a, b_ in zip(r1, r2))


def test_two_lanes_equal_one_lane(run):
    """Two concurrent lanes of one image each (their own plans, quantise launches and tile choices) give the one-lane detections bit for
    bit: int32 sums are exact and the BF16 tiles share one K order, so nothing depends on the batch composition."""
    _two_lanes_equal_one_lane(run)


# ---- 64 x 96, B = 3: the same replay where height != width and the batch is odd
def test_rect_plan_is_64_by_96_with_three_images(run_rect):
    """The fixture is what it says: buffers of 2 : 3 pictures at every depth, the route and upsample shapes included."""
    plan, specs = run_rect["plan"], run_rect["specs"]
    assert (plan.B, plan.H, plan.W) == (RECT_B, RECT_H, RECT_W) and int(plan.flags.item()) == 0
    assert tuple(plan.front_q.shape) == (1, RECT_B, RECT_H // 2, RECT_W // 2, 64)
    shapes = {tuple(plan.layer_out[specs[i].name].shape[2:4]) for i in ir.int8_layers(specs)}
    assert shapes == {(RECT_H // f, RECT_W // f) for f in (4, 8, 16, 32)}, shapes
    assert sorted(run_rect["scales"]) == sorted(ir.scale_names(specs))


def test_rect_front_is_the_bf16_engines_and_is_quantised_by_definition(run_rect):
    _front_is_the_bf16_engines_and_is_quantised_by_definition(run_rect)


def test_rect_all_int8_layers_bit_identical_to_the_numpy_replay(run_rect):
    """64 x 96, B = 3: every layer_out buffer and the three head inputs against the chained numpy replay, wired by the architecture."""
    _all_int8_layers_bit_identical_to_the_numpy_replay(run_rect)


def test_rect_two_lanes_of_2_and_1_equal_one_lane(run_rect):
    """An uneven lane split: the lanes take 2 and 1 of the three images."""
    _two_lanes_equal_one_lane(run_rect)


def test_changed_scale_repacks_and_changes_the_output(run):
    """(last: it leaves the network with another scale)"""
    net, x, eng, specs = run["net"], run["x"], run["eng"], run["specs"]
    name = specs[30].name
    before = net.forward_cat(x).clone()
    gen = eng.generation
    assert torch.equal(net.forward_cat(x), before) and eng.generation == gen
    net.int8_scales = dict(net.int8_scales, **{name: net.int8_scales[name] * 1.5})
    after = net.forward_cat(x)
    assert eng.generation == gen + 1, "a changed scale must re-pack"
    assert not torch.equal(after, before) and bool(torch.isfinite(after).all())
