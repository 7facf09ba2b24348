"""Time the GPU JPEG encoder (yolo_v3_amd/jpeg.py encode_batch) against PIL in the same run: batches of 1, 8, 64 and 256 images at
416x416 and 640x480, for 4:2:0 at quality 75 and 4:4:4 at quality 95.  The images are photographic-like content (smooth structure
plus mild noise), resident on the device for the GPU passes and in host memory for PIL.  Settings, interleaved round by round,
the median of the rounds reported:
  gpu_device   the device time between two events around `submit_encode` (nine kernels, the record upload, the length copy)
  gpu_wall     `encode_batch` up to the bytes in host memory: the above, the one read of the lengths, the packing of the files
               on the device and their copy to the host
  pil_1        ``Image.fromarray(a).save(buffer, "JPEG", quality=, subsampling=)`` in the calling thread
  pil_8        the same on an eight-thread pool
and, once per case, the device time of each kernel from a profiled call.  One JSON line per (size, mode, batch size).

    python tools/jpeg_enc_bench.py [--rounds 7] [--warmup 2] [--bs 1 8 64 256]
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from yolo_v3_amd import jpeg        # noqa: E402

KERNELS = ("enc_layout_kernel", "enc_coef_kernel", "enc_size_kernel", "enc_scan_kernel", "enc_zero_kernel", "enc_emit_kernel",
           "enc_count_kernel", "enc_finish_kernel", "enc_scatter_kernel")
PIL_SUB = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def pictures(w, h, n, seed=7):
    """n distinct uint8 RGB images: low-frequency structure with mild noise (16 base images, cycled with a shift)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = []
    for i in range(min(n, 16)):
        planes = [127 + 90 * np.sin(xx / rng.uniform(20, 90) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(20, 90) + rng.uniform(0, 6)) for _ in range(3)]
        base.append(np.clip(np.stack(planes, -1) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8))
    return [np.ascontiguousarray(np.roll(base[i % len(base)], i // len(base) * 8, axis=1)) for i in range(n)]


def pil_file(a, quality, sub):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=PIL_SUB[sub])
    return b.getvalue()


def gpu_pass(dev_images, quality, sub):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    job = jpeg.submit_encode(dev_images, quality=quality, subsampling=sub)
    e1.record()
    files = job.finish()
    wall = time.perf_counter() - t0
    torch.cuda.synchronize()
    return wall * 1e3, e0.elapsed_time(e1), files


def pil_pass(images, quality, sub, pool):
    t0 = time.perf_counter()
    enc = lambda a: pil_file(a, quality, sub)
    out = list(pool.map(enc, images)) if pool is not None else [enc(a) for a in images]
    assert len(out) == len(images)
    return (time.perf_counter() - t0) * 1e3


def kernel_split(dev_images, quality, sub):
    """Device microseconds per kernel of one call, or None where the profiler gives no device times."""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            jpeg.encode_batch(dev_images, quality=quality, subsampling=sub)
            torch.cuda.synchronize()
        split = {}
        for ev in prof.key_averages():
            for k in KERNELS:
                if k in ev.key:
                    us = getattr(ev, "device_time_total", None)
                    if us is None:
                        us = getattr(ev, "cuda_time_total", 0.0)
                    split[k] = round(split.get(k, 0.0) + float(us), 1)
                    break
        return split or None
    except Exception as e:                               # the split is an extra: the rates do not depend on it
        return {"error": repr(e)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    rate = lambda n, ms: round(n * 1e3 / ms, 1)
    for (w, h) in ((416, 416), (640, 480)):
        for (sub, quality) in (("4:2:0", 75), ("4:4:4", 95)):
            for bs in a.bs:
                images = pictures(w, h, bs)
                dev_images = [torch.from_numpy(im).cuda() for im in images]
                files = gpu_pass(dev_images, quality, sub)[2]
                assert files[0] == pil_file(images[0], quality, sub) and files[-1] == pil_file(images[-1], quality, sub)
                samples = {k: [] for k in ("gpu_wall", "gpu_device", "pil_1", "pil_8")}
                with ThreadPoolExecutor(max_workers=8) as pool:
                    for r in range(a.warmup + a.rounds):
                        got = {}
                        got["gpu_wall"], got["gpu_device"], _ = gpu_pass(dev_images, quality, sub)
                        got["pil_1"] = pil_pass(images, quality, sub, None)
                        got["pil_8"] = pil_pass(images, quality, sub, pool)
                        if r >= a.warmup:
                            for k, v in got.items():
                                samples[k].append(v)
                med = {k: float(np.median(v)) for k, v in samples.items()}
                out = {"shape": [h, w], "subsampling": sub, "quality": quality, "bs": bs, "file_bytes": int(np.mean([len(f) for f in files])),
                       "rounds": a.rounds}
                for k in samples:
                    out[k + "_ms"] = round(med[k], 3)
                    out["min_max_" + k + "_ms"] = [round(min(samples[k]), 3), round(max(samples[k]), 3)]
                    out[k + "_images_per_s"] = rate(bs, med[k])
                out["kernel_us"] = kernel_split(dev_images, quality, sub)
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
