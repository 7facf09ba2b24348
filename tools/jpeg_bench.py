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

--progressive: both sources' pixels are encoded again by PIL at quality 90, 4:2:0, once with ``progressive=True`` and once as the
baseline twin, and for each source at bs = 16 / 64 / 256, all in this one run and interleaved round by round: decode_batch with
``progressive=True`` on the progressive bytes (wall and device time), PIL on one and on eight threads on the same progressive
bytes, and the serial baseline stage on the twins; then, from one profiled call each, the device time of entropy_prog_kernel
and of the twins' entropy_kernel<0>.  One JSON line per (source, batch size).

    python tools/jpeg_bench.py --progressive [--rounds 5] [--warmup 1]
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

KERNELS = ("layout_prog_kernel", "entropy_prog_kernel", "layout_kernel", "entropy_kernel<0>", "entropy_kernel<1>", "entropy_kernel", "idct_kernel", "colour_kernel")


def sources(kind, bs):
    if kind == "photo":
        return [open(os.path.join(REPO, "tests", "golden", "x_wing_0001.jpg"), "rb").read()] * bs
    with tempfile.TemporaryDirectory() as root:
        lst = loader_bench.write_files(root)
        files = [open(p.strip(), "rb").read() for p in open(lst)]
    return [files[i % len(files)] for i in range(bs)]


def gpu_pass(datas, entropy="serial", progressive=False):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = jpeg.decode_batch(datas, entropy=entropy, progressive=progressive)
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


def kernel_split(datas, entropy="serial", progressive=False):
    """Device microseconds per kernel of one call, or None where the profiler gives no device times."""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            jpeg.decode_batch(datas, entropy=entropy, progressive=progressive)
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


def encode_again(data, progressive):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(evaluate.read_image_rgb(io.BytesIO(data))).save(b, "JPEG", quality=90, subsampling=2, progressive=progressive)
    return b.getvalue()


def progressive_main(a):
    rate = lambda n, ms: round(n * 1e3 / ms, 1)
    for src in ("synth", "photo"):
        base = [(encode_again(d, True), encode_again(d, False)) for d in sources(src, 1 if src == "photo" else 64)]
        for bs in (16, 64, 256):
            prog = [base[i % len(base)][0] for i in range(bs)]
            twin = [base[i % len(base)][1] for i in range(bs)]
            ref = evaluate.read_image_rgb(io.BytesIO(prog[0]))
            assert np.array_equal(jpeg.decode_batch(prog[:1], progressive=True)[0].cpu().numpy(), ref)
            assert np.array_equal(jpeg.decode_batch(twin[:1])[0].cpu().numpy(), ref)
            samples = {k: [] for k in ("prog_wall", "prog_device", "twin_wall", "twin_device", "pil_1", "pil_8")}
            with ThreadPoolExecutor(max_workers=8) as pool:
                for r in range(a.warmup + a.rounds):
                    got = {}
                    got["prog_wall"], got["prog_device"] = gpu_pass(prog, progressive=True)
                    got["twin_wall"], got["twin_device"] = gpu_pass(twin)
                    got["pil_1"] = pil_pass(prog, None)
                    got["pil_8"] = pil_pass(prog, pool)
                    if r >= a.warmup:
                        for k, v in got.items():
                            samples[k].append(v)
            med = {k: float(np.median(v)) for k, v in samples.items()}
            info, rec = jpeg.parse_ex(prog[0])
            coded = int(np.mean([sum(r.scans[i].length for i in range(r.nscans)) for r in (jpeg.parse_ex(d)[1] for d in prog)]))
            out = {"src": src, "shape": list(ref.shape[:2]), "bs": bs, "progressive_file_bytes": int(np.mean([len(d) for d in prog])),
                   "twin_file_bytes": int(np.mean([len(d) for d in twin])), "coded_bytes": coded, "scans": rec.nscans,
                   "levels": rec.nlevels, "rounds": a.rounds}
            for k in samples:
                out[k + "_ms"] = round(med[k], 3)
                out["min_max_" + k + "_ms"] = [round(min(samples[k]), 3), round(max(samples[k]), 3)]
            for k in ("prog_wall", "twin_wall", "pil_1", "pil_8"):
                out[k + "_images_per_s"] = rate(bs, med[k])
            out["prog_kernel_us"] = kernel_split(prog, progressive=True)
            out["twin_kernel_us"] = kernel_split(twin)
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--src", choices=("synth", "photo"), default="synth")
    ap.add_argument("--entropy", choices=("serial", "parallel", "both"), default="serial")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--progressive", action="store_true")
    a = ap.parse_args()
    if a.progressive:
        return progressive_main(a)
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
