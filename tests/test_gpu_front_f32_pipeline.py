"""The persistent exact-fp32 front kernels (csrc/conv_front_f32.hip, csrc/conv_res64_f32.hip) defer each tile's epilogue into the next
tile: these tests check them BIT FOR BIT against the two-launch path where that pipeline has its edges -- workgroups with one, two,
three and four tiles (prologue without a pending epilogue, the drain after the loop), tile counts just below and above a multiple of
the CU count, large and non-square pictures, and two fused launches in a row on the same buffers."""
import pytest
import torch

from yolo_v3_amd import _ffi, synth

pytestmark = pytest.mark.gpu


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _net(H, W):
    from yolo_v3_amd import YoloNet, WeightManager
    stream = synth.weight_stream()
    net = YoloNet((W, H)).eval()
    assert WeightManager(net).load_stream(stream) == stream.size
    net = net.cuda()
    net.math_mode = _ffi.F32
    return net


def _pair(B, H, W, seed, switch, layer):
    """`layer`'s output with the fused kernel switched off and on (NaN-filled before the fused run: every element must be written),
    plus a second fused run on the same buffers."""
    net = _net(H, W)
    x = torch.from_numpy(synth.images(B, max(H, W), seed)[:, :, :H, :W].copy()).cuda()
    eng = net.engine(_ffi.F32)
    outs, dets = [], []
    try:
        for fused in (False, True):
            setattr(eng, switch, fused)
            eng._plans = {}
            d, plan = eng.forward(x)
            assert getattr(plan, switch.replace("fuse_", "fused_")) == fused
            if fused:
                plan.layer_out[layer].fill_(float("nan"))
                d, plan = eng.forward(x)
            outs.append(plan.layer_out[layer].clone())
            dets.append(d.clone())
        d, plan = eng.forward(x)                                          # again, same plan, same buffers
        outs.append(plan.layer_out[layer].clone())
        dets.append(d.clone())
    finally:
        setattr(eng, switch, True)
        eng._plans = {}
    assert outs[0].shape == (B, H // 2, W // 2, 64) and outs[0].dtype == torch.float32
    assert torch.isfinite(outs[1]).all()
    for o in outs[1:]:
        assert torch.equal(outs[0], o), "%d elements differ, max |d| %g" % (int((outs[0] != o).sum()), float((outs[0] - o).abs().max()))
    for d in dets[1:]:
        assert torch.equal(dets[0], d)


def _tiles(B, H, W):
    return B * (W // 32) * (H // 16)                     # 8 x 16 tiles of the 208-class layer: the same count for both kernels


# (B as a function of the CU count, H, W): at 32 x 32 a picture is two tiles
SHAPES = [
    (lambda n: 1, 64, 64),                               # 8 tiles: eight workgroups with one tile each
    (lambda n: n // 2 - 1, 32, 32),                      # two tiles short of one round: one tile per workgroup
    (lambda n: n // 2 + 1, 32, 32),                      # two tiles past one round: two workgroups walk two tiles
    (lambda n: n - 1, 32, 32),                           # two tiles short of two rounds: one or two tiles
    (lambda n: (3 * n) // 2 - 1, 32, 32),                # three tiles (odd) for most workgroups, two for the last two
    (lambda n: (3 * n) // 2 + 1, 32, 32),                # three tiles, four for two workgroups
    (lambda n: 1, 608, 608),
    (lambda n: 2, 224, 544),                             # non-square
]


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_fused_front_f32_pipeline_bitwise(shape):
    bf, H, W = SHAPES[shape]
    B = max(1, bf(_ncu()))
    assert _tiles(B, H, W) >= 1
    _pair(B, H, W, 21 + shape, "fuse_front", "feature.mlist.1")


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_fused_res64_f32_pipeline_bitwise(shape):
    bf, H, W = SHAPES[shape]
    B = max(1, bf(_ncu()))
    assert _tiles(B, H, W) >= 1
    _pair(B, H, W, 41 + shape, "fuse_res64", "feature.mlist.2.conv2")
