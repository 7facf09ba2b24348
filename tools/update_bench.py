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

With --optimizer adam | adamw the same protocol times Adam / AdamW (torch's default hyper-parameters on the same two groups):

  torch       torch.nn.utils.clip_grad_norm_(params, 1000) + torch.optim.Adam.step(), torch's defaults (foreach kernels)
  torch_fused the same with torch.optim.Adam(fused=True)
  separate    yolo_v3_amd.optim.clip_grad_norm_(params, 1000) + yolo_v3_amd.optim.Adam.step()
  clipped     yolo_v3_amd.optim.Adam.step_clipped(1000)

and each row also carries `step_bytes`, the bytes the Adam step itself must move -- 28 per element (read g, p, exp_avg, exp_avg_sq;
write p, exp_avg, exp_avg_sq), 36 with --amsgrad -- and `step_TBps`, those bytes over the row's median time (the norm's read of g
and, where the gradients are rewritten, the clip's traffic come on top: `bytes` counts them as for SGD).

    python tools/update_bench.py [--batch 16] [--rounds 9] [--math bf16] [--optimizer sgd|adam|adamw] [--amsgrad]
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
ADAM = {"adam": (torch.optim.Adam, optim.Adam), "adamw": (torch.optim.AdamW, optim.AdamW)}


def two_groups(net, cls, **hyper):
    """The reference's two param groups; without `hyper`, its SGD settings."""
    backbone = {id(p) for p in net.feature.parameters()}
    groups = [{"params": [p for p in net.parameters() if id(p) not in backbone], "lr": LR},
              {"params": list(net.feature.parameters()), "lr": BACKBONE_LR}]
    return cls(groups, LR, **hyper) if hyper else cls(groups, LR, weight_decay=WD, momentum=MOMENTUM)


def summary(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--math", choices=tuple(MATH), default="bf16")
    ap.add_argument("--optimizer", choices=("sgd",) + tuple(ADAM), default="sgd")
    ap.add_argument("--amsgrad", action="store_true", help="Adam / AdamW with amsgrad (36 bytes per element)")
    a = ap.parse_args()
    if a.amsgrad and a.optimizer == "sgd":
        ap.error("--amsgrad goes with --optimizer adam or adamw")
    net = YoloNet((416, 416), numClass=80)
    WeightManager(net).load_stream(trained_like_stream(80))
    net = net.to(DEV).train()
    net.backprop, net.backprop_math = True, MATH[a.math]
    x = torch.from_numpy(synth.images(a.batch, 416, 7)).to(DEV)
    tg = torch.from_numpy(R.random_rows(5, a.batch, 30, 80, (0.03, 0.8)))
    params = list(net.parameters())
    if a.optimizer == "sgd":
        opt_torch, opt_sep, opt_clip = two_groups(net, torch.optim.SGD), two_groups(net, optim.SGD), two_groups(net, optim.SGD)
    else:
        theirs, ours = ADAM[a.optimizer]
        opt_torch, opt_fused = two_groups(net, theirs, amsgrad=a.amsgrad), two_groups(net, theirs, amsgrad=a.amsgrad, fused=True)
        opt_sep, opt_clip = two_groups(net, ours, amsgrad=a.amsgrad), two_groups(net, ours, amsgrad=a.amsgrad)

    def backward():
        net.zero_grad(set_to_none=True)
        net(x, tg).backward()

    def torch_update():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt_torch.step()

    def separate_update():
        optim.clip_grad_norm_(params, MAX_NORM)
        opt_sep.step()

    def torch_fused_update():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt_fused.step()

    updates = {"torch": torch_update, "separate": separate_update, "clipped": lambda: opt_clip.step_clipped(MAX_NORM)}
    words, step_bytes = dict(WORDS), None
    if a.optimizer != "sgd":
        updates = {"torch": torch_update, "torch_fused": torch_fused_update, "separate": updates["separate"], "clipped": updates["clipped"]}
        step_words = 9 if a.amsgrad else 7
        words = {"torch": step_words + 3, "torch_fused": step_words + 3, "separate": step_words + 3, "clipped": step_words + 1}
    backward()
    torch.cuda.synchronize()
    saved = [p.grad.detach().clone() for p in params]
    grads = [p.grad for p in params]
    n_elem = sum(p.numel() for p in params)
    norm0 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in saved)))
    out = {"batch": a.batch, "math": a.math, "tensors": len(params), "elements": n_elem, "grad_norm": round(norm0, 3),
           "max_norm": MAX_NORM, "rounds": a.rounds}
    if a.optimizer != "sgd":
        step_bytes = step_words * 4 * n_elem
        out.update(optimizer=a.optimizer, amsgrad=a.amsgrad, step_bytes=step_bytes)

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
            r["bytes"] = words[k] * 4 * n_elem
            r["GBps"] = round(r["bytes"] / r["median_ms"] / 1e6, 1)
            if step_bytes:
                r["step_TBps"] = round(step_bytes / r["median_ms"] / 1e9, 3)
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
        for rival in ("torch", "torch_fused")[:1 if a.optimizer == "sgd" else 2]:
            spread = max(out[mode][k]["max_ms"] - out[mode][k]["min_ms"] for k in (rival, "clipped"))
            out["clipped_faster_than_%s_beyond_spread_%s" % (rival, mode)] = bool(out[mode][rival]["median_ms"] - out[mode]["clipped"]["median_ms"] > spread)
    assert all(bool(torch.isfinite(p).all()) for p in params), "a parameter left the finite range"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
