"""Time one training step at 416x416 (net(x, target) + loss.backward(), net.backprop = True, .train()) at bs=8 and bs=16, against the
same network run by torch's own modules in fp32 (F.conv2d / F.batch_norm on MIOpen, tests/train_ref.forward) in the same process.
7 interleaved rounds, median reported; then one profiled step of ours split by kernel class.

    python tools/train_bench.py [--batches 8 16] [--rounds 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import train_ref as T                      # noqa: E402
from tests import yolo_loss_ref as R                  # noqa: E402
from tests.helpers import trained_like_stream         # noqa: E402
from yolo_v3_amd import YoloNet, WeightManager, synth  # noqa: E402

DEV = "cuda:0"


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def kernel_classes(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    cls = {}
    for ev in prof.key_averages():
        n = ev.key
        k = ("conv fwd" if "conv_gemm<0>" in n else "conv dgrad" if "conv_gemm<1>" in n else "conv wgrad" if "conv_gemm<2>" in n
             or "wgrad_reduce" in n else "BN / act" if any(s in n for s in ("channel_partials", "finalize", "bn_act", "eval_stats"))
             else "loss" if "yolo" in n.lower() or "loss" in n.lower() else "other")
        cls[k] = cls.get(k, 0.0) + getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)) / 1e3
    return {k: round(v, 3) for k, v in sorted(cls.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    net = YoloNet((416, 416), numClass=80)
    WeightManager(net).load_stream(trained_like_stream(80))
    net = net.to(DEV).train()
    net.backprop = True
    sd_gpu = {k: v.detach().clone() for k, v in net.state_dict().items()}
    out = {}
    for B in a.batches:
        x = torch.from_numpy(synth.images(B, 416, 7)).to(DEV)
        tg = torch.from_numpy(R.random_rows(5, B, 30, 80, (0.03, 0.8)))

        def ours():
            net.zero_grad(set_to_none=True)
            net(x, tg).backward()

        def torch_modules():
            logits, _, _ = T.forward(sd_gpu, x, True, torch.float32)
            torch.autograd.backward(logits, [torch.ones_like(l) * 1e-3 for l in logits])

        ours(); torch_modules()
        t_ours, t_torch = [], []
        for _ in range(a.rounds):
            t_ours.append(timed(ours))
            t_torch.append(timed(torch_modules))
        out[B] = dict(ours_ms=float(np.median(t_ours)), torch_miopen_fp32_ms=float(np.median(t_torch)))
        try:
            out[B]["ours_by_kernel_class_ms"] = kernel_classes(ours)
        except Exception as e:                       # (the profiler is a diagnostic only)
            out[B]["ours_by_kernel_class_ms"] = "profiler unavailable: %s" % e
        print(B, json.dumps(out[B]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
