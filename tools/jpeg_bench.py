"""Time the GPU JPEG decoder (yolo_v3_amd/jpeg.py decode_batch) against PIL in the same run: images per second for one batch size
and one kind of source per invocation.

  --src synth   tools/loader_bench.py's 64 synthetic 640x480 quality-90 files (4:2:0), cycled to the batch size
  --src photo   tests/golden/x_wing_0001.jpg (1280x546, 4:2:0), replicated
Settings, interleaved round by round (one pass of each per round), the median of the rounds reported:
  gpu        decode_batch on file bytes already in memory: wall time up to a device synchronise (host parse, the one upload, four
             kernels, the status read), and the device time between two events around the same call; with --entropy both, one
             pass with the serial entropy stage and one with the parallel one in every round
  pil_1      PIL (``evaluate.read_image_rgb`` on the same bytes) in the calling thread
  pil_8      the same on an eight-thread pool
and, once per entropy stage, the device time of each kernel from a profiled call (torch.profiler), as the split (the parallel
stage's kernel is the instance entropy_kernel<1>).  One JSON line; with --entropy both the gpu figures come per stage, under
"serial" and "parallel".

    python tools/jpeg_bench.py --bs 64 --src synth [--entropy serial|parallel|both] [--rounds 9] [--warmup 2]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from yolo_v3_amd import evaluate, jpeg        # noqa: E402
from tools import loader_bench                # noqa: E402

KERNELS = ("layout_kernel", "entropy_kernel<0>", "entropy_kernel<1>", "entropy_kernel", "idct_kernel", "colour_kernel")


def sources(kind, bs):
    if kind == "photo":
        return [open(os.path.join(REPO, "tests", "golden", "x_wing_0001.jpg"), "rb").read()] * bs
    with tempfile.TemporaryDirectory() as root:
        lst = loader_bench.write_files(root)
        files = [open(p.strip(), "rb").read() for p in open(lst)]
    return [files[i % len(files)] for i in range(bs)]


def gpu_pass(datas, entropy="serial"):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = jpeg.decode_batch(datas, entropy=entropy)
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert not any(out.fallback) and not any(out.handed_over)
    return wall * 1e3, e0.elapsed_time(e1)


def pil_pass(datas, pool):
    t0 = time.perf_counter()
    read = lambda d: evaluate.read_image_rgb(io.BytesIO(d))
    out = list(pool.map(read, datas)) if pool is not None else [read(d) for d in datas]
    assert len(out) == len(datas)
    return (time.perf_counter() - t0) * 1e3


def kernel_split(datas, entropy="serial"):
    """Device microseconds per kernel of one call, or None where the profiler gives no device times."""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            jpeg.decode_batch(datas, entropy=entropy)
            torch.cuda.synchronize()
        split = {}
        for ev in prof.key_averages():
            for k in KERNELS:                            # the first name that fits: the instance, where the profiler shows it
                if k in ev.key:
                    us = getattr(ev, "device_time_total", None)
                    if us is None:
                        us = getattr(ev, "cuda_time_total", 0.0)
                    split[k] = round(split.get(k, 0.0) + float(us), 1)
                    break
        return split or None
    except Exception as e:                               # the split is an extra: the rates above do not depend on it
        return {"error": repr(e)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--src", choices=("synth", "photo"), default="synth")
    ap.add_argument("--entropy", choices=("serial", "parallel", "both"), default="serial")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    modes = ("serial", "parallel") if a.entropy == "both" else (a.entropy,)
    datas = sources(a.src, a.bs)
    ref = evaluate.read_image_rgb(io.BytesIO(datas[0]))
    for m in modes:
        assert np.array_equal(jpeg.decode_batch(datas[:1], entropy=m)[0].cpu().numpy(), ref)
    samples = {"pil_1": [], "pil_8": []}
    for m in modes:
        samples[m + "_wall"], samples[m + "_device"] = [], []
    with ThreadPoolExecutor(max_workers=8) as pool:
        for r in range(a.warmup + a.rounds):
            got = {}
            for m in modes:                              # interleaved: one pass of every setting per round
                got[m + "_wall"], got[m + "_device"] = gpu_pass(datas, m)
            got["pil_1"] = pil_pass(datas, None)
            got["pil_8"] = pil_pass(datas, pool)
            if r >= a.warmup:
                for k, v in got.items():
                    samples[k].append(v)
    med = {k: float(np.median(v)) for k, v in samples.items()}
    rate = lambda ms: round(a.bs * 1e3 / ms, 1)

    def gpu_fields(m):
        return {"gpu_wall_ms": round(med[m + "_wall"], 3), "gpu_device_ms": round(med[m + "_device"], 3),
                "gpu_images_per_s": rate(med[m + "_wall"]), "gpu_device_images_per_s": rate(med[m + "_device"]),
                "min_max_gpu_wall_ms": [round(min(samples[m + "_wall"]), 3), round(max(samples[m + "_wall"]), 3)],
                "min_max_gpu_device_ms": [round(min(samples[m + "_device"]), 3), round(max(samples[m + "_device"]), 3)],
                "kernel_us": kernel_split(datas, m)}
    out = {"src": a.src, "shape": list(ref.shape[:2]), "bs": a.bs, "file_bytes": int(np.mean([len(d) for d in datas])),
           "entropy": a.entropy, "pil_1_ms": round(med["pil_1"], 3), "pil_8_ms": round(med["pil_8"], 3),
           "pil_1_images_per_s": rate(med["pil_1"]), "pil_8_images_per_s": rate(med["pil_8"]),
           "min_max_pil_8_ms": [round(min(samples["pil_8"]), 3), round(max(samples["pil_8"]), 3)], "rounds": a.rounds}
    if len(modes) == 1:
        out.update(gpu_fields(modes[0]))
    else:
        for m in modes:
            out[m] = gpu_fields(m)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
