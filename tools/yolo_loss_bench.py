"""Time the YOLO loss at 416x416, batch 64 (csrc/yololoss.hip): the kernels alone (loss only, loss + dL/dlogits) on the three heads'
NHWC logits, and net(x, target) against net(x) in exact F32 and F32H2.  Variants run interleaved, round after round; each line gives
the median and the spread over rounds of the per-call time, plus the effective bandwidth of the kernels and the bytes of the logits
plan that the plane modes add.

    python tools/yolo_loss_bench.py [--batch 64] [--rounds 7] [--iters 10] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from yolo_v3_amd import YoloNet, WeightManager, _ffi, synth, yololayer  # noqa: E402
from tests import yolo_loss_ref as R                                       # noqa: E402


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="skip the network (for a kernel trace)")
    a = ap.parse_args()
    B, dev = a.batch, torch.device("cuda:0")
    torch.cuda.set_device(dev)
    C = 80
    tg = torch.from_numpy(R.random_rows(7, B, 50, C, (0.01, 0.9), n_valid_lo=50)).to(dev)
    heads = []
    for k, (h, mask) in enumerate(((13, [6, 7, 8]), (26, [3, 4, 5]), (52, [0, 1, 2]))):
        x = torch.from_numpy(synth.uniform(50 + k, 3, B * h * h * 255, -4.0, 4.0).reshape(B, h, h, 255)).to(dev)
        heads.append((x, h, mask, torch.empty_like(x)))
    out = torch.empty(3 * yololayer.HEAD_OUT_BYTES, device=dev, dtype=torch.uint8)
    n_logits = sum(x.numel() for x, _, _, _ in heads)

    def kernels(grad):
        def run():
            for k, (x, h, mask, g) in enumerate(heads):
                yololayer.launch_loss(x, (h * h * 255, 255, 1), tg, h, h, C, 416, R.ANCHORS, mask,
                                      out[k * yololayer.HEAD_OUT_BYTES:], g if grad else None)
        return run

    variants = {"kernels_loss": kernels(False), "kernels_loss_grad": kernels(True)}
    if not a.kernels_only:
        variants.update(network_variants(B, dev, tg))
    for fn in variants.values():                  # warm-up: plans, packing, workspaces
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, a.iters if k.startswith("kernels") else max(2, a.iters // 4)))
    res = {}
    for k, v in times.items():
        v = np.array(v)
        res[k] = dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()))
        line = "%-18s median %8.3f ms  [%8.3f .. %8.3f]" % (k, res[k]["median_ms"], v.min(), v.max())
        if k.startswith("kernels"):
            nbytes = n_logits * 4 * (2 if k.endswith("grad") else 1)
            res[k]["GB_per_s"] = nbytes / (res[k]["median_ms"] * 1e-3) / 1e9
            line += "  %.0f GB/s effective (%.0f MB: logits read%s)" % (res[k]["GB_per_s"], nbytes / 1e6,
                                                                       " + gradient written" if k.endswith("grad") else "")
        print(line)
    if not a.kernels_only:
        net = variants["net_f32"].net
        net.math_mode = _ffi.F32H2
        eng = net.engine()
        base = eng.plan(B, 416, 416).bytes_allocated()
        extra = eng.plan(B, 416, 416, logits=True).bytes_allocated()
        res["f32h2_plan_bytes"], res["f32h2_logits_plan_bytes"] = base, extra
        print("F32H2 plan %.2f GB; the logits plan adds %.2f GB" % (base / 1e9, extra / 1e9))
    print("logits: %d floats (%.0f MB)" % (n_logits, n_logits * 4 / 1e6))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def network_variants(B, dev, tg):
    """net(x) and net(x, target) in exact F32 and F32H2 (SW-1 weights, seeded images)."""
    net = YoloNet((416, 416)).eval()
    stream = synth.weight_stream()
    WeightManager(net).load_stream(stream)
    net = net.cuda()
    ximg = torch.from_numpy(synth.images(B, 416, 99)).to(dev)
    tg_cpu = tg.cpu()

    def net_call(mode, loss):
        def run():
            net.math_mode = mode
            with torch.no_grad():
                net(ximg, tg_cpu) if loss else net(ximg)
        return run

    variants = {"net_f32": net_call(_ffi.F32, False), "net_f32_loss": net_call(_ffi.F32, True),
                "net_f32h2": net_call(_ffi.F32H2, False), "net_f32h2_loss": net_call(_ffi.F32H2, True)}
    variants["net_f32"].net = net
    return variants


if __name__ == "__main__":
    main()
