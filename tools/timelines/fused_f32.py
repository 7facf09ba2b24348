"""Per-wave cycle split of workgroup 17 of the two exact-fp32 fused kernels -- conv_front_f32_kernel and conv_res64_f32_kernel -- per
tile: top barrier (with the waits in front of it) | deferred epilogue | first layer or 1x1 (with the image writes) | mid barrier | 3x3.
Needs a -DYV3_TIMELINE build (tools/build_variant.sh tl "-DYV3_TIMELINE"; YV3_MEASURE=1 YV3_LIB=.../libyv3_tl.so): the split replaces
the first floats of both outputs (results INVALID).  416x416, bs from BB (64)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from yolo_v3_amd import YoloNet, WeightManager, synth, _ffi
torch.cuda.set_device(0)
B = int(os.environ.get("BB", "64"))
net = YoloNet((416, 416)).eval(); WeightManager(net).load_stream(synth.weight_stream()); net = net.cuda()
eng = net.engine(_ffi.F32); eng.ensure_packed()
plan = eng.plan(B, 416, 416)
assert plan.fused_front and plan.fused_res64
x = torch.rand(B, 3, 416, 416, device="cuda")
for _ in range(3):
    eng.run_front(plan, x)
torch.cuda.synchronize()
for name, layer, conv1 in (("conv_front_f32", "feature.mlist.1", "first layer"), ("conv_res64_f32", "feature.mlist.2.conv2", "1x1")):
    d = plan.layer_out[layer].reshape(-1)[:64].cpu().tolist()
    print("%s, workgroup 17, %d tiles; cycles per tile (s_memtime):" % (name, int(d[6])))
    print("  wave | top barrier | epilogue | %11s | mid barrier |   3x3 | sum | whole loop / tiles" % conv1)
    for w in range(8):
        v = d[8 * w: 8 * w + 8]
        print("  %4d | %11.0f | %8.0f | %11.0f | %11.0f | %5.0f | %5.0f | %6.0f" % (w, v[0], v[1], v[2], v[3], v[4], sum(v[:5]), v[5] / max(v[6], 1)))
