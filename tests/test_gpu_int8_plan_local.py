"""Every int8 launch of the three I8 plans DESIGN.md 8g's table was timed on -- 416x416 bs=16, 608x608 bs=16, 416x416 bs=64, one lane,
SW-1 weights, synth.images -- checked on the tensors the GPU itself fed it (-m gpu, through the C-ABI), bit for bit: integer sums are
exact, there is no tolerance.  The scales come from net.calibrate_int8 on the first two images of each picture size and serve every batch
size of that size (realistic, not optimal).  After one forward of the plan:

  * status and reach: status word 0; on 256 CUs the plan's kernel lines are exactly the table's row (REACH below: tile, channel tiles,
    loop, with the number of layers on each) -- the ping-pong, rolling and four-wave launches the published numbers rest on.  The engine
    sets no descriptor field that changes an int8 choice in a one-lane plan; on another CU count the lines are printed instead;
  * wiring: each int8 descriptor's input pointers and cin_up name the producers int8_ref.wiring derives from the architecture;
  * value: at sampled output pixels, all channels -- the four corners of the first and of the last image, the launch's last row, one
    random row of every row tile of 256 rows and 64 random rows (fixed seed) -- the k x k input windows are gathered from the plan's
    own layer_out buffers with torch indexing on the device (upsample + concat and the residual included; only the windows travel to
    the host) and int8_ref.layer_at_pixels evaluates the definition on them, with weights quantised by int8_ref.quantize_weights
    from the module's fp32 parameters, the folded BatchNorm and the scales (not the packed image, not the descriptor's alpha / beta);
  * full tensor, independent tile: a copy of the descriptor is relaunched with forced tile code 2 (128x128_W8; code 1, 256x128_W8, where
    the plan already runs 128x128_W8) into a buffer filled with -128 (bf16 output: NaN) with sentinels behind it: every element written,
    the sentinels intact, the tile asked for was run, and the output equals the plan's buffer.  tests/test_gpu_int8_conv.py holds the
    forced tiles whole against the definition on grids with many tiles, so samples + equality cover every output of every launch.  The
    two 64-channel layers have one tile only (128x64: the relaunch repeats it; test_gpu_int8_conv.py's 64-channel grid case holds it);
  * the three layers in front of the heads (bf16 integers out) under the same checks;
  * non-vacuity: every launch's sampled reference has more than 20 distinct values, the median over the 68 launches is above 50; each
    layer's share of sampled outputs at +-127 is printed.

All 68 launches of every plan are checked in full, at bs=64 too: on an MI355X the bs=64 test takes 0.5 s (38 692 sampled pixels) against
1.9 s at 416x416 bs=16 (13 325 pixels; it quantises the weights for both) and 1.3 s at 608x608 bs=16 (22 942), so no subset was needed.
Whole network at 416x416 bs=16: Detector(lanes=2) -- 8 images per lane, other kernels than for 16 -- equals lanes=1, and the logits of a
bs=2 forward (all 128x128_W8 / 128x64 plain) equal rows 0 and 1 of the bs=16 forward."""
import collections
import time

import numpy as np
import pytest
import torch

from yolo_v3_amd import _ffi, arch, synth, Detector
from tests import int8_ref as ir
from tests.helpers import load_sw1_net, desc_inputs_by_pointer, copy_desc, relaunch_desc, relaunch_desc_i8

pytestmark = pytest.mark.gpu

I8, BF16, F32 = _ffi.I8, _ffi.BF16, _ffi.F32
SEED = 2029
N_RANDOM = 64

# (size, batch) -> {kernel line: int8 layers on it} as conv_select.cpp chooses at 256 CUs
REACH = {
    (416, 64): {"256x256_PP4 nt=1 pingpong": 12, "192x256_PP4 nt=2 pingpong": 12, "192x256_PP4 nt=4 pingpong": 8, "256x128_W4 nt=1 plain": 11,
                "256x128_W4 nt=2 plain": 11, "256x128_W4_ROLL nt=1 rolling": 3, "256x128_W8_PP6 nt=1 pingpong": 1, "256x128_W8_PP6 nt=4 pingpong": 7,
                "128x128_W8 nt=2 plain": 1, "128x64 nt=1 plain": 2},
    (416, 16): {"192x256_PP4 nt=1 pingpong": 12, "256x128_W8_PP6 nt=1 pingpong": 11, "256x128_W8_PP6 nt=4 pingpong": 12, "256x128_W4_ROLL nt=1 rolling": 3,
                "128x128_W8 nt=1 plain": 1, "128x128_W8 nt=2 plain": 12, "128x128_W8 nt=4 plain": 7, "128x128_W8 nt=8 plain": 8, "128x64 nt=1 plain": 2},
    (608, 16): {"192x256_PP4 nt=1 pingpong": 12, "192x256_PP4 nt=2 pingpong": 12, "256x128_W4 nt=1 plain": 11, "256x128_W4_ROLL nt=1 rolling": 3,
                "256x128_W8_PP6 nt=2 pingpong": 11, "256x128_W8_PP6 nt=8 pingpong": 8, "128x128_W8 nt=1 plain": 1, "128x128_W8 nt=2 plain": 1,
                "128x128_W8 nt=4 plain": 7, "128x64 nt=1 plain": 2},
}
assert all(sum(v.values()) == 68 for v in REACH.values())


def _line(full):
    """tile, channel tiles and loop of a kernel line."""
    return " ".join(full.split()[:3])


class _Nets:
    """Per picture size, made on first use and then read only: the calibrated network in I8 mode, its scales, the folded BatchNorm of
    every int8 layer and the weights as the definition quantises them."""

    def __init__(self, stream):
        self.stream, self.by_size = stream, {}

    def get(self, size):
        if size not in self.by_size:
            specs = arch.conv_specs(80)
            net = load_sw1_net(self.stream, size).cuda()
            x16 = torch.from_numpy(synth.images(16, size, 4242 + size)).cuda()
            scales = dict(net.calibrate_int8([x16[:2].contiguous()]))
            net.math_mode = I8
            f32 = net.engine(F32)                       # packed by the calibration: the folded BatchNorm of every layer
            g = ir.wiring(specs)
            fold, qw = {}, {}
            for i in ir.int8_layers(specs):
                src, route, _ = g[i]
                s_in = ir.input_scales(specs[i].cin, scales[specs[src].name], specs[src].cout if route is not None else 0,
                                       scales[specs[route].name] if route is not None else None)
                fold[i] = (f32.packed[i].alpha.cpu().numpy(), f32.packed[i].beta.cpu().numpy())
                q, sw = ir.quantize_weights(net.get_submodule(specs[i].name).conv.weight.detach().cpu().numpy(), s_in)
                qw[i] = (q.astype(np.int8), sw)          # (integers in [-127, 127]: kept as bytes)
            self.by_size[size] = dict(net=net, x16=x16, scales=scales, specs=specs, g=g, fold=fold, qw=qw)
        return self.by_size[size]


@pytest.fixture(scope="module")
def nets(sw1_stream):
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    return _Nets(sw1_stream)


def _images(c, size, B):
    """The batch of a plan: the 16 images the scales' two came from, followed by further ones."""
    if B <= 16:
        return c["x16"][:B].contiguous()
    return torch.cat((c["x16"], torch.from_numpy(synth.images(B - 16, size, 777 + size)).cuda()))


def _sample_rows(M, rng):
    """Rows of the launch's [M, cout] output: one random row of every row tile of 256, the last row, and N_RANDOM random ones."""
    starts = np.arange(0, M, 256, dtype=np.int64)
    in_tile = starts + rng.integers(0, np.minimum(256, M - starts))
    return np.concatenate((in_tile, [M - 1], rng.integers(0, M, N_RANDOM)))


def _pixels(B, ho, wo, rng):
    rows = _sample_rows(B * ho * wo, rng)
    pix = np.stack((rows // (ho * wo), rows // wo % ho, rows % wo), axis=1)
    corners = [(b, y, x) for b in (0, B - 1) for y in (0, ho - 1) for x in (0, wo - 1)]
    pix = np.unique(np.concatenate((np.array(corners, dtype=np.int64), pix)), axis=0)
    assert len(pix) >= 64 and {tuple(p) for p in corners} <= {tuple(p) for p in pix.tolist()} and (pix[-1] == (B - 1, ho - 1, wo - 1)).all()
    assert len(np.unique((pix[:, 0] * ho * wo + pix[:, 1] * wo + pix[:, 2]) // 256)) == -(-(B * ho * wo) // 256), "a row tile of 256 has no sample"
    return pix


def _windows(x, x2, pix, k, stride):
    """ir.gather_patches on the device: [P, k, k, C] int8 on the host.  x, x2: [B, H, W, C] int8 device tensors."""
    H, W = (x2 if x2 is not None else x).shape[1:3]
    b, yi, xi, inside = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ir.patch_index(pix, k, stride, H, W))
    if x2 is None:
        p = x[b, yi, xi]
    else:
        p = torch.cat((x[b, yi // 2, xi // 2], x2[b, yi, xi]), dim=3)
    return (p * inside[..., None].to(torch.int8)).cpu().numpy()


def _check_plan(nets, size, B):
    t0 = time.time()
    c = nets.get(size)
    net, specs, g, scales = c["net"], c["specs"], c["g"], c["scales"]
    x = _images(c, size, B)
    eng = net.engine()
    assert eng.dtype == I8
    t1 = time.time()
    _, plan = eng.forward(x, logits=True)
    torch.cuda.synchronize()
    t_fwd = time.time() - t1
    assert plan.B == B and int(plan.flags.item()) == 0
    kernels = plan.kernels()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    names = desc_inputs_by_pointer(plan)
    rng = np.random.default_rng(SEED + size + B)

    def tensor(i):                                          # conv i's output as the int8 layers read it: [B, h, w, c] int8 on the device
        t = plan.front_q if i == ir.I8_FIRST - 1 else plan.layer_out[specs[i].name]
        assert t.dtype == torch.int8 and t.shape[0] == 1
        return t[0]

    reach, spread, sat, fails, n_pix, bf16_out = collections.Counter(), [], [], [], 0, 0
    launches = [(j, plan.desc_spec[j]) for j in range(plan.first_desc, plan.n_desc) if plan.descs[j].dtype == I8]
    assert [i for _, i in launches] == ir.int8_layers(specs) and len(launches) == 68
    for j, i in launches:
        d, sp, full = plan.descs[j], specs[i], kernels[j - plan.first_desc]
        line = _line(full)
        reach[line] += 1
        what = "%dx%d bs=%d launch %d %s (conv %d) [%s]" % (size, size, B, j, sp.name, i, full)
        # ---- wiring
        src, route, res = g[i]
        want_names = (specs[src].name, specs[route].name if route is not None else None, specs[res].name if res is not None else None)
        assert names(d) == want_names and d.cin_up == (specs[src].cout if route is not None else 0), (what, names(d), d.cin_up)
        assert (d.cin, d.cout, d.k, d.stride, d.B) == (sp.cin, sp.cout, sp.k, sp.stride, B), what
        to_head = not specs[i + 1].bn
        assert d.out_dtype == (BF16 if to_head else I8), what
        bf16_out += to_head
        out = plan.layer_out[sp.name]
        ho, wo = out.shape[2:4]
        n = B * ho * wo * sp.cout
        assert out.dtype == (torch.bfloat16 if to_head else torch.int8) and out.numel() == n and out.data_ptr() == d.y, what
        assert (ho, wo) == ((d.H - 1) // sp.stride + 1, (d.W - 1) // sp.stride + 1), what
        # ---- value at sampled pixels
        pix = _pixels(B, ho, wo, rng)
        dev = [torch.from_numpy(pix[:, a]).cuda() for a in range(3)]
        win = _windows(tensor(src), tensor(route) if route is not None else None, pix, sp.k, sp.stride)
        assert win.shape == (len(pix), sp.k, sp.k, sp.cin), (what, win.shape)
        res_q = tensor(res)[dev[0], dev[1], dev[2]].cpu().numpy() if res is not None else None
        alpha, beta = c["fold"][i]
        want = ir.layer_at_pixels(win, None, None, alpha, beta, scales[sp.name], res_q, scales[specs[res].name] if res is not None else None, qw_sw=c["qw"][i])
        got = out[0][dev[0], dev[1], dev[2]].float().cpu().numpy()
        n_pix += len(pix)
        distinct = len(np.unique(want))
        spread.append(distinct)
        sat.append(float((np.abs(want) == 127).mean()))
        assert distinct > 20, "%s: the sampled reference has %d distinct values: the launch is checked on nothing" % (what, distinct)
        bad = np.argwhere(got != want)
        if bad.size:
            p = tuple(bad[0])
            fails.append("%s: %d of %d sampled outputs differ from the definition, first at pixel (b, y, x) = %s channel %d: got %g, want %g" % (
                what, len(bad), want.size, tuple(int(v) for v in pix[p[0]]), p[1], got[p], want[p]))
            break                                           # the first failing launch names the layer and the kernel line
        # ---- the whole tensor on another tile
        tile = line.split()[0]
        code = _ffi.TILE_256x128_W8 if tile == "128x128_W8" else _ffi.TILE_128x128_W8
        cpy = copy_desc(d)
        cpy.options |= code << _ffi.OPT_TILE_SHIFT
        other = _ffi.conv2d_kernel(cpy).split()[0]
        if sp.cout % 128:
            assert tile == other == "128x64", (what, other)           # (64 output channels: the one tile there is)
        else:
            assert other == ("256x128_W8" if code == _ffi.TILE_256x128_W8 else "128x128_W8") and other != tile, (what, other)
        again = relaunch_desc(cpy, n, what + ", forced " + other, torch.bfloat16) if to_head else relaunch_desc_i8(cpy, n, what + ", forced " + other)
        a, b_ = (again.view(torch.int16), out.reshape(-1).view(torch.int16)) if to_head else (again, out.reshape(-1))
        if not torch.equal(a, b_):
            fails.append("%s: %d of %d outputs differ from the same launch on tile %s" % (what, int((a != b_).sum()), n, other))
            break
        assert int(plan.flags.item()) == 0, "%s: status word %d" % (what, int(plan.flags.item()))
    assert not fails, "\n".join(fails)
    assert bf16_out == 3
    print("i8 plan local | %dx%d bs=%d | %d CUs | 68 int8 launches, %d sampled pixels (all channels), 68 whole-tensor relaunches | forward %.2f s, test %.1f s"
          % (size, size, B, ncu, n_pix, t_fwd, time.time() - t0))
    print("    kernel lines (layers): " + "; ".join("%s (%d)" % kv for kv in sorted(reach.items())))
    print("    distinct sampled values per launch: min %d median %d | share at +-127 per layer, %%: %s" % (
        min(spread), int(np.median(spread)), " ".join("%.2f" % (100.0 * s) for s in sat)))
    assert np.median(spread) > 50, "the activations do not use the int8 range: the samples check little"
    if ncu == 256:
        assert dict(reach) == REACH[(size, B)], "the plan's kernel lines are not the timed plan's: %s" % dict(reach)
    return plan, x


def test_i8_plan_416_bs16_launch_by_launch_and_across_batch_sizes(nets):
    """416x416 bs=16, all 68 int8 launches; then the whole network: the logits of a bs=2 forward of images 0 and 1 (every int8 layer on
    128x128_W8 / 128x64 plain) equal rows 0 and 1 of the bs=16 forward -- nothing depends on the batch's composition."""
    plan, x = _check_plan(nets, 416, 16)
    eng = nets.get(416)["net"].engine()
    _, p2 = eng.forward(x[:2].contiguous(), logits=True)
    torch.cuda.synchronize()
    assert p2 is not plan and p2.B == 2 and int(p2.flags.item()) == 0
    lines = {_line(k) for j, k in zip(range(p2.first_desc, p2.n_desc), p2.kernels()) if p2.descs[j].dtype == I8}
    print("i8 plan local | 416x416 bs=2 int8 kernel lines: %s" % "; ".join(sorted(lines)))
    assert all(ln.split()[0] in ("128x128_W8", "128x64") and ln.endswith("plain") for ln in lines), lines
    assert len(plan.logits) == len(p2.logits) == 3
    for (l16, h, w), (l2, h2, w2) in zip(plan.logits, p2.logits):
        assert (h, w) == (h2, w2) and l16.dtype == l2.dtype == torch.float32 and bool(torch.isfinite(l2).all())
        a, b_ = l16.reshape(16, -1)[:2].contiguous(), l2.reshape(2, -1)
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), "%dx%d head: %d logits of images 0 and 1 differ between bs=16 and bs=2" % (
            h, w, int((a != b_).sum()))


def test_i8_plan_608_bs16_launch_by_launch(nets):
    _check_plan(nets, 608, 16)


def test_i8_plan_416_bs64_launch_by_launch(nets):
    """(the scales are those of the bs=16 test: calibrated on images 0 and 1)"""
    _check_plan(nets, 416, 64)


def test_i8_two_lanes_of_8_equal_one_lane_of_16(nets):
    """416x416 bs=16: Detector(lanes=2) runs 8 images per lane, for which the selector picks other kernels than for 16 (asserted), and
    gives lanes=1's detections and boxes bit for bit."""
    c = nets.get(416)
    net, x = c["net"], c["x16"]
    with torch.no_grad():
        one = Detector(net, 16, 416, 416, 0.05, 0.4, lanes=1)
        r1 = one(x)
        two = Detector(net, 16, 416, 416, 0.05, 0.4, lanes=2)
        r2 = two(x)
    assert (one.lanes, two.lanes) == (1, 2) and one.engine.dtype == two.engine.dtype == I8
    assert [p.B for p in two.lane_plans] == [8, 8] and [p.B for p in one.lane_plans] == [16]
    k1, k2 = one.lane_plans[0].kernels(), two.lane_plans[0].kernels()
    differ = sum(_line(a) != _line(b_) for a, b_ in zip(k1, k2))
    print("i8 plan local | 416x416 bs=16: %d of %d launches run another kernel line in a lane of 8" % (differ, len(k1)))
    assert len(k1) == len(k2) and differ > 0, "the lanes run the one-lane plan's kernels: the equality compares a kernel with itself"
    assert bool(torch.isfinite(one.dets).all()) and torch.equal(one.dets, two.dets)
    assert len(r1) == len(r2) == 16 and all(torch.equal(a, b_) for a, b_ in zip(r1, r2))
    print("i8 plan local | boxes per image: %s" % [int(t.shape[0]) if t.numel() else 0 for t in r1])
