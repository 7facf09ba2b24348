"""Time the training loader (yolo_v3_amd/augment.py TrainBatches) on files: 64 synthetic 640x480 JPEGs (quality 90, from a seed) with
their label files in a temporary directory, bs 16, dim 416, whole epochs ending in a device synchronise.

  defaults   read and decode in the calling thread, every epoch (what TrainBatches did before it had options)
  workers    workers=8: the next batches' files are decoded on threads
  resident   cache_bytes holding the whole list, measured from the second epoch on: no file is read, no pixel uploaded
  defaults_gpu / workers_gpu   the first two with decode="gpu": the JPEGs are decoded on the GPU (yolo_v3_amd/jpeg.py), one batch ahead
  *_par      (--entropy parallel | both) the two decode="gpu" settings with entropy="parallel", the self-synchronising entropy stage;
             --entropy parallel replaces the serial ones by them, --entropy both times both in the same rounds
  *+step     the four above (and the *_par ones) with a stand-in training step after every batch: fp32 matrix products on the current stream, sized at
             start-up to --step-ms of device time and only enqueued (as a training loop enqueues its step), so that the setting's
             ms per batch minus --step-ms is what the loader adds to a step it can overlap with
Rounds are interleaved (one epoch of every setting per round); per setting the median, minimum and maximum of the per-epoch
ms per batch, the batches per second of the median, the host's share (time inside ``next()``, before the synchronise; median, minimum and maximum too) and the
bytes uploaded per batch as the code counts them (``augment.counters``).  One JSON line per setting.

    python tools/loader_bench.py [--rounds 9] [--warmup 2] [--workers 8] [--entropy serial|parallel|both]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from yolo_v3_amd import augment as aug        # noqa: E402

N_IMAGES, BS, DIM, H, W = 64, 16, 416, 480, 640


def write_files(root, seed=0, n_labels=8):
    from PIL import Image
    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, "labels"))
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    paths = []
    for i in range(N_IMAGES):
        # colour ramps with a few random blocks and mild noise: a JPEG of a photograph's size, not of white noise
        fx, fy = rng.uniform(0.5, 3.0, 2)
        img = np.stack([127 + 120 * np.sin(xx * fx / 100.0 + i), 127 + 120 * np.cos(yy * fy / 80.0), (xx + yy + 37 * i) % 256], -1)
        for _ in range(12):
            y0, x0 = rng.randint(0, H - 40), rng.randint(0, W - 40)
            img[y0:y0 + rng.randint(20, 200), x0:x0 + rng.randint(20, 200)] = rng.randint(0, 256, 3)
        img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
        p = os.path.join(root, "images", "img%03d.jpg" % i)
        Image.fromarray(img).save(p, format="JPEG", quality=90)
        paths.append(p)
        rows = np.column_stack([rng.randint(0, 80, n_labels), rng.uniform(0.2, 0.8, (n_labels, 2)), rng.uniform(0.05, 0.4, (n_labels, 2))])
        np.savetxt(os.path.join(root, "labels", "img%03d.txt" % i), rows)
    lst = os.path.join(root, "train.txt")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    return lst


def make_step(step_ms):
    """A function that enqueues about ``step_ms`` of matrix products on the current stream, and the device ms it measured for it."""
    a = torch.randn(4096, 4096, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        a @ a
    e0.record()
    for _ in range(10):
        a @ a
    e1.record()
    torch.cuda.synchronize()
    reps = max(1, int(round(step_ms / (e0.elapsed_time(e1) / 10))))

    def step():
        for _ in range(reps):
            a @ a
    e0.record()
    step()
    e1.record()
    torch.cuda.synchronize()
    return step, e0.elapsed_time(e1)


def epoch(loader, step=None):
    """One epoch: (wall ms per batch up to the synchronise, host ms per batch inside next(), upload bytes per batch)."""
    before = dict(aug.counters)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host, n, it = 0.0, 0, iter(loader)
    while True:
        h0 = time.perf_counter()
        batch = next(it, None)
        host += time.perf_counter() - h0
        if batch is None:
            break
        n += 1
        if step is not None:
            step()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return wall * 1e3 / n, host * 1e3 / n, (aug.counters["upload_bytes"] - before["upload_bytes"]) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--step-ms", type=float, default=80.0)
    ap.add_argument("--entropy", choices=("serial", "parallel", "both"), default="serial")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as root:
        lst = write_files(root)
        make = lambda **kw: aug.TrainBatches(lst, BS, (DIM, DIM), seed=1, **kw)
        loaders = {"defaults": make(), "workers": make(workers=a.workers), "resident": make(cache_bytes=make().decoded_bytes())}
        if a.entropy != "parallel":
            loaders.update({"defaults_gpu": make(decode="gpu"), "workers_gpu": make(workers=a.workers, decode="gpu")})
        if a.entropy != "serial":
            loaders.update({"defaults_gpu_par": make(decode="gpu", entropy="parallel"),
                            "workers_gpu_par": make(workers=a.workers, decode="gpu", entropy="parallel")})
        step, step_ms = make_step(a.step_ms)
        steps = {}
        for k in [k for k in loaders if k != "resident"]:
            loaders[k + "+step"] = make(workers=loaders[k].workers, decode=loaders[k].decode, entropy=loaders[k].entropy)
            steps[k + "+step"] = step
        epoch(loaders["resident"])                         # the first epoch fills the arena
        assert loaders["resident"].resident_images() == N_IMAGES
        samples = {k: [] for k in loaders}
        for r in range(a.warmup + a.rounds):
            for k, loader in loaders.items():              # interleaved: every setting once per round
                s = epoch(loader, steps.get(k))
                if r >= a.warmup:
                    samples[k].append(s)
        for k, v in samples.items():
            wall, host = sorted(s[0] for s in v), sorted(s[1] for s in v)
            med = float(np.median(wall))
            print(json.dumps({"setting": k, "bs": BS, "dim": DIM, "src": "%dx%d jpeg q90" % (W, H), "images": N_IMAGES,
                              "workers": loaders[k].workers, "cache_bytes": loaders[k].cache_bytes, "decode": loaders[k].decode,
                              "entropy": loaders[k].entropy if loaders[k].decode == "gpu" else None,
                              "ms_per_batch": round(med, 3), "min_ms": round(wall[0], 3), "max_ms": round(wall[-1], 3),
                              "batches_per_s": round(1e3 / med, 1), "host_ms_per_batch": round(float(np.median(host)), 3),
                              "host_min_ms": round(host[0], 3), "host_max_ms": round(host[-1], 3),
                              "upload_bytes_per_batch": int(np.median([s[2] for s in v])), "rounds": a.rounds,
                              "step_ms": round(step_ms, 3) if k in steps else None}))


if __name__ == "__main__":
    main()
