"""Time the update step -- gradient clipping + SGD with momentum and weight decay -- over the 80-class net's own parameters (222
tensors, ~62 M elements) at 416x416 bs=16, BF16, after one real backward, three ways in the same process:

  torch       torch.nn.utils.clip_grad_norm_(params, 1000) + torch.optim.SGD.step(), torch's defaults (foreach kernels)
  separate    yolo_v3_amd.optim.clip_grad_norm_(params, 1000) + yolo_v3_amd.optim.SGD.step()
  clipped     yolo_v3_amd.optim.SGD.step_clipped(1000)

Each optimizer follows the reference's get_optimizer (two param groups, momentum 0.9, weight decay 5e-4) and owns its momentum
buffers; all three update the same parameters.  Interleaved rounds, median reported with the min / max of the rounds:

  alone       device events around the update only, the GPU idle when the call starts: the host's share (argument checks, pointer
              tables, launches) is inside.  The gradients of the real backward are restored before each call, outside the events
  queued      the same events with ~4 ms of other GPU work queued in front, so that the host runs ahead as it does in a training
              step: the device time of the update's kernels
  step        wall clock of zero_grad + net(x, target) + backward + update, synchronised, beside the same step without an update

GB/s is over the bytes each must move, in fp32 words per parameter element: torch and `separate` 8 (norm: read g; clip: read and
write g; update: read g, p, buf, write p, buf), `clipped` 6 (no rewrite of g).

    python tools/update_bench.py [--batch 16] [--rounds 9] [--math bf16]
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

from tests import yolo_loss_ref as R                  # noqa: E402
from tests.helpers import trained_like_stream         # noqa: E402
from yolo_v3_amd import YoloNet, WeightManager, synth, optim, F32, BF16, BF16_ACT  # noqa: E402

MATH = {"f32": F32, "bf16": BF16, "bf16_act": BF16_ACT}
DEV = "cuda:0"
MAX_NORM, LR, BACKBONE_LR, WD, MOMENTUM = 1000.0, 1e-3, 1e-4, 5e-4, 0.9
WORDS = {"torch": 8, "separate": 8, "clipped": 6}


def two_groups(net, cls):
    backbone = {id(p) for p in net.feature.parameters()}
    return cls([{"params": [p for p in net.parameters() if id(p) not in backbone], "lr": LR},
                {"params": list(net.feature.parameters()), "lr": BACKBONE_LR}], LR, weight_decay=WD, momentum=MOMENTUM)


def summary(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--math", choices=tuple(MATH), default="bf16")
    a = ap.parse_args()
    net = YoloNet((416, 416), numClass=80)
    WeightManager(net).load_stream(trained_like_stream(80))
    net = net.to(DEV).train()
    net.backprop, net.backprop_math = True, MATH[a.math]
    x = torch.from_numpy(synth.images(a.batch, 416, 7)).to(DEV)
    tg = torch.from_numpy(R.random_rows(5, a.batch, 30, 80, (0.03, 0.8)))
    params = list(net.parameters())
    opt_torch, opt_sep, opt_clip = two_groups(net, torch.optim.SGD), two_groups(net, optim.SGD), two_groups(net, optim.SGD)

    def backward():
        net.zero_grad(set_to_none=True)
        net(x, tg).backward()

    def torch_update():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt_torch.step()

    def separate_update():
        optim.clip_grad_norm_(params, MAX_NORM)
        opt_sep.step()

    updates = {"torch": torch_update, "separate": separate_update, "clipped": lambda: opt_clip.step_clipped(MAX_NORM)}
    backward()
    torch.cuda.synchronize()
    saved = [p.grad.detach().clone() for p in params]
    grads = [p.grad for p in params]
    n_elem = sum(p.numel() for p in params)
    norm0 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in saved)))
    out = {"batch": a.batch, "math": a.math, "tensors": len(params), "elements": n_elem, "grad_norm": round(norm0, 3),
           "max_norm": MAX_NORM, "rounds": a.rounds}

    # ---- the update alone, device events
    filler = torch.zeros(1 << 28, device=DEV)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def event_ms(f, queued):
        torch._foreach_copy_(grads, saved)
        torch.cuda.synchronize()
        for _ in range(8 if queued else 0):
            filler.add_(1.0)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):                         # (the first step creates the momentum buffers and sizes the workspaces)
        for f in updates.values():
            event_ms(f, True)
    for mode in ("alone", "queued"):
        times = {k: [] for k in updates}
        for _ in range(a.rounds):
            for k, f in updates.items():
                times[k].append(event_ms(f, mode == "queued"))
        out[mode] = {}
        for k, v in times.items():
            r = summary(v)
            r["bytes"] = WORDS[k] * 4 * n_elem
            r["GBps"] = round(r["bytes"] / r["median_ms"] / 1e6, 1)
            out[mode][k] = r
        print(mode, json.dumps(out[mode]), flush=True)
    del filler
    try:                                       # (the profiler is a diagnostic only)
        from torch.profiler import profile, ProfilerActivity
        out["kernels_ms"] = {}
        for k, f in updates.items():
            torch._foreach_copy_(grads, saved)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                f()
                torch.cuda.synchronize()
            out["kernels_ms"][k] = {ev.key[:60]: [ev.count, round(getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)) / 1e3, 4)]
                                    for ev in prof.key_averages()}
    except Exception as e:
        out["kernels_ms"] = "profiler unavailable: %s" % e

    # ---- the whole training step, wall clock
    steps = {"no_update": lambda: None}
    steps.update(updates)
    whole = {k: [] for k in steps}
    for f in steps.values():
        backward()
        f()
    for _ in range(a.rounds):
        for k, f in steps.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            backward()
            f()
            torch.cuda.synchronize()
            whole[k].append((time.perf_counter() - t) * 1e3)
    out["step"] = {k: summary(v) for k, v in whole.items()}
    for k in updates:
        out["step"][k]["update_share_ms"] = round(out["step"][k]["median_ms"] - out["step"]["no_update"]["median_ms"], 4)
    for mode in ("alone", "queued"):           # the acceptance rule: the medians differ by more than max - min of either side
        spread = max(out[mode][k]["max_ms"] - out[mode][k]["min_ms"] for k in ("torch", "clipped"))
        out["clipped_faster_than_torch_beyond_spread_" + mode] = bool(out[mode]["torch"]["median_ms"] - out[mode]["clipped"]["median_ms"] > spread)
    assert all(bool(torch.isfinite(p).all()) for p in params), "a parameter left the finite range"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
