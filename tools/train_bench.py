"""Time one training step at 416x416 (net(x, target) + loss.backward(), net.backprop = True, .train()) at bs=8 and bs=16, for each
net.backprop_math in --math (f32: exact fp32; bf16: bf16 convolution operands; bf16_act: bf16 with the activations stored in bf16
only), against the same network run by torch's own modules
in fp32 (F.conv2d / F.batch_norm on MIOpen, tests/train_ref.forward) and, with bf16 in --math, the same under
torch.autocast("cuda", torch.bfloat16), all in the same process.  7 interleaved rounds, median reported; then one profiled step of
each of ours split by kernel class (conv classes also in TFLOP/s of the products they compute), and the device memory each of ours
holds between forward and backward (torch.cuda.memory_allocated with the loss alive, minus its value before the forward).

--input-grad instead times our step with net.input_grad off and on (x.requires_grad), interleaved in the same way, and the layer-0
input-gradient kernel alone (yv3_train_conv0_dgrad[_bf16]) beside layer 0's wgrad launch, which reads the same dz: device events
around 50 launches that rotate over enough dz buffers to exceed the 256 MiB Infinity Cache, and the rate over the bytes the kernel
must move (dz read once, dx written).

--state backbone_eval_frozen instead times the fine-tuning step on a frozen eval-mode Darknet-53 (tests/train_states.py: heads trainable
in train mode) with net.frozen_prefix off and on -- the 52 frozen convolutions on the training kernels, or on the inference engine --
interleaved in the same way, for each --math, with the kernel-class split and the held memory of both, and the device memory the
prefix engine keeps for good (its packed weights and one plan per (B, H, W)).

    python tools/train_bench.py [--batches 8 16] [--rounds 7] [--math f32 bf16 bf16_act] [--input-grad] [--state backbone_eval_frozen]
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
from tests import train_states as S                   # noqa: E402
from tests import yolo_loss_ref as R                  # noqa: E402
from tests.helpers import trained_like_stream         # noqa: E402
from yolo_v3_amd import YoloNet, WeightManager, synth, arch, backprop, _ffi, F32, BF16, BF16_ACT  # noqa: E402

MATH = {"f32": F32, "bf16": BF16, "bf16_act": BF16_ACT}

DEV = "cuda:0"
# kernels only the inference engine launches (net.frozen_prefix): its convolutions, their Winograd input transforms, the widening of a
# handed-over bf16 plane
PREFIX_KERNELS = ("conv_igemm_f32", "conv_gemm1x1_f32", "conv_planes", "conv_front", "conv_res64", "conv_wino4", "wino4_input", "wino_input",
                  "conv0_kernel", "conv0_mfma", "merge_planes")


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
        k = ("prefix (inference kernels)" if any(s in n for s in PREFIX_KERNELS) else "input dgrad" if "conv0_dgrad" in n else "conv fwd" if "conv_gemm<0>" in n or "conv_bf16<0," in n else "conv dgrad" if "conv_gemm<1>" in n or "conv_bf16<1," in n
             else "conv wgrad" if "conv_gemm<2>" in n or "conv_bf16<2," in n or "wgrad_reduce" in n
             else "cast" if "to_bf16" in n else "weight pack" if "pack_weight" in n
             else "BN / act" if any(s in n for s in ("channel_partials", "finalize", "bn_act", "eval_stats", "bias_bwd"))
             else "loss" if "yolo" in n.lower() or "loss" in n.lower() else "other")
        cls[k] = cls.get(k, 0.0) + getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)) / 1e3
    return {k: round(v, 3) for k, v in sorted(cls.items())}


def held_mb(net, x, tg, math):
    """MB of device memory one step holds between its forward and its backward."""
    net.backprop_math = math
    net.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    loss = net(x, tg)
    held = torch.cuda.memory_allocated() - before
    loss.backward()
    return round(held / 1e6, 1)


def step_gflop(B, size=416):
    """GFLOP of one forward's convolutions (2 M N K over all layers); dgrad and wgrad compute the same products once more each."""
    tot = 0
    for sp, (ho, wo) in zip(arch.conv_specs(80), arch.conv_output_hw(size, 80)):
        tot += 2 * B * ho * wo * sp.cout * sp.cin * sp.k * sp.k
    return tot / 1e9


def event_ms(launch, n_buffers, reps=50):
    """Mean device time of launch(i % n_buffers) over `reps` launches (after one warm-up pass over the buffers)."""
    for i in range(n_buffers):
        launch(i)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(reps):
        launch(i % n_buffers)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def conv0_dgrad_alone(B, math, size=416, cout=32):
    """The input-gradient kernel and layer 0's wgrad on [B, size, size, cout] dz -> dict of times and the dgrad's rate."""
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    m = backprop.MATH[math]
    bf = m.bf16_operands
    dz_bytes = B * size * size * cout * (2 if bf else 4)
    dx_bytes = B * 3 * size * size * 4
    nbuf = max(2, -(-600 * 2 ** 20 // dz_bytes))
    g = torch.Generator(device=DEV).manual_seed(1)
    dzs = [torch.randn(B, size, size, cout, device=DEV, generator=g).to(torch.bfloat16 if bf else torch.float32) for _ in range(nbuf)]
    x = torch.randn(B, 3, size, size, device=DEV, generator=g)
    xin = x.to(torch.bfloat16) if bf else x
    w = torch.randn(cout, 3, 3, 3, device=DEV, generator=g) / 27 ** 0.5
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    dgrad, wgrad = backprop.entry(lib, m.conv0_dgrad), backprop.entry(lib, m.conv_wgrad)
    nw = backprop.entry(lib, m.conv_wgrad_ws)(B, size, size, 3, cout, 3, 1)
    ws = torch.empty(nw, device=DEV, dtype=torch.uint8)
    t_d = event_ms(lambda i: _ffi.check(dgrad(dzs[i].data_ptr(), w.data_ptr(), dx.data_ptr(), B, size, size, cout, s)), nbuf)
    t_w = event_ms(lambda i: _ffi.check(wgrad(xin.data_ptr(), None, dzs[i].data_ptr(), dw.data_ptr(), B, size, size, 3, 0, cout, 3, 1, 1,
                                              ws.data_ptr(), nw, s)), nbuf)
    return {"conv0_dgrad_ms": round(t_d, 4), "conv0_dgrad_bytes": dz_bytes + dx_bytes,
            "conv0_dgrad_TBps": round((dz_bytes + dx_bytes) / t_d / 1e9, 3), "layer0_wgrad_ms": round(t_w, 4), "dz_buffers": nbuf}


def input_grad_cost(net, a):
    """--input-grad: the step with net.input_grad off / on, interleaved, and the new kernel alone."""
    out = {}
    net.input_grad = True
    for B in a.batches:
        x = torch.from_numpy(synth.images(B, 416, 7)).to(DEV)
        tg = torch.from_numpy(R.random_rows(5, B, 30, 80, (0.03, 0.8)))
        out[B] = {}
        for m in a.math:
            def step(want_x, math=MATH[m]):
                net.backprop_math = math
                net.zero_grad(set_to_none=True)
                xin = x.clone().requires_grad_(True) if want_x else x
                net(xin, tg).backward()
            fns = {"off_ms": lambda: step(False), "on_ms": lambda: step(True)}
            for f in fns.values():
                f()
            times = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, f in fns.items():
                    times[k].append(timed(f))
            r = {k: round(float(np.median(v)), 3) for k, v in times.items()}
            r["spread_ms"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
            r.update(conv0_dgrad_alone(B, MATH[m]))
            out[B][m] = r
            print(B, m, json.dumps(r), flush=True)
    print(json.dumps(out))


def frozen_prefix_cost(net, a):
    """--state: the step under the state with net.frozen_prefix off / on, interleaved."""
    S.STATES[a.state].apply(net)
    n = backprop.frozen_prefix_ops(net)
    out = {"state": a.state, "prefix_ops": n}
    for B in a.batches:
        x = torch.from_numpy(synth.images(B, 416, 7)).to(DEV)
        tg = torch.from_numpy(R.random_rows(5, B, 30, 80, (0.03, 0.8)))
        out[B] = {}
        for m in a.math:
            def step(on, math=MATH[m]):
                net.backprop_math, net.frozen_prefix = math, on
                net.zero_grad(set_to_none=True)
                net(x, tg).backward()
            fns = {"off_ms": lambda: step(False), "on_ms": lambda: step(True)}
            net.repack()                                   # (the prefix engine of the batch before: its plan is not this one's)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            for f in fns.values():
                f()
            times = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, f in fns.items():
                    times[k].append(timed(f))
            r = {k: round(float(np.median(v)), 3) for k, v in times.items()}
            r["spread_ms"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
            net.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            r["prefix_engine_MB"] = round((torch.cuda.memory_allocated() - base) / 1e6, 1)      # packed weights + the plan's buffers
            for on in (False, True):
                net.frozen_prefix = on
                r["held_MB_" + ("on" if on else "off")] = held_mb(net, x, tg, MATH[m])
                try:
                    r["by_kernel_class_ms_" + ("on" if on else "off")] = kernel_classes(fns["on_ms" if on else "off_ms"])
                except Exception as e:                   # (the profiler is a diagnostic only)
                    r["by_kernel_class_ms_" + ("on" if on else "off")] = "profiler unavailable: %s" % e
            out[B][m] = r
            print(B, m, json.dumps(r), flush=True)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--math", nargs="+", choices=tuple(MATH), default=["f32"])
    ap.add_argument("--input-grad", action="store_true", help="time the step with net.input_grad off and on, and the layer-0 dgrad alone")
    ap.add_argument("--state", choices=("all_train", "backbone_eval_frozen"), default="all_train",
                    help="backbone_eval_frozen: time the fine-tuning step with net.frozen_prefix off and on")
    a = ap.parse_args()
    net = YoloNet((416, 416), numClass=80)
    WeightManager(net).load_stream(trained_like_stream(80))
    net = net.to(DEV).train()
    net.backprop = True
    if a.input_grad:
        return input_grad_cost(net, a)
    if a.state != "all_train":
        return frozen_prefix_cost(net, a)
    sd_gpu = {k: v.detach().clone() for k, v in net.state_dict().items()}
    out = {}
    for B in a.batches:
        x = torch.from_numpy(synth.images(B, 416, 7)).to(DEV)
        tg = torch.from_numpy(R.random_rows(5, B, 30, 80, (0.03, 0.8)))

        def ours(math):
            def step():
                net.backprop_math = math
                net.zero_grad(set_to_none=True)
                net(x, tg).backward()
            return step

        def torch_modules():
            logits, _, _ = T.forward(sd_gpu, x, True, torch.float32)
            torch.autograd.backward(logits, [torch.ones_like(l) * 1e-3 for l in logits])

        def torch_autocast():
            with torch.autocast("cuda", torch.bfloat16):
                logits, _, _ = T.forward(sd_gpu, x, True, torch.float32)
            torch.autograd.backward(logits, [torch.ones_like(l) * 1e-3 for l in logits])

        fns = {"ours_%s_ms" % m: ours(MATH[m]) for m in MATH if m in a.math}
        fns["torch_miopen_fp32_ms"] = torch_modules
        if "bf16" in a.math or "bf16_act" in a.math:
            fns["torch_autocast_bf16_ms"] = torch_autocast
        for f in fns.values():
            f()
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                times[k].append(timed(f))
        out[B] = {k: float(np.median(v)) for k, v in times.items()}
        for m in a.math:
            out[B]["ours_%s_held_MB" % m] = held_mb(net, x, tg, MATH[m])
        gf = step_gflop(B)
        for m in a.math:
            key = "ours_%s_by_kernel_class_ms" % m
            try:
                cls = kernel_classes(fns["ours_%s_ms" % m])
                out[B][key] = cls
                out[B]["ours_%s_conv_tflops" % m] = {c: round(gf / cls[c], 1) for c in ("conv fwd", "conv dgrad", "conv wgrad")
                                                     if cls.get(c)}
            except Exception as e:                   # (the profiler is a diagnostic only)
                out[B][key] = "profiler unavailable: %s" % e
        print(B, json.dumps(out[B]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
