"""Time the reference's ExtraAugmentations on the GPU (yolo_v3_amd/extra_augment.py, csrc/extra_augment.hip): 640x480 sources,
bs 16 and 64.

  per operation  yv3_extra_augment (its six launches) with every image running that one operation at its most expensive
                 setting, on sources already on the device; "copy" is the program without steps
  sampled        the same entry point on the programs sample_extra draws for seeds 0 .. bs-1
  end to end     extra_augment_batch from host numpy images with those programs: packing, the one upload, the launches
  augment        the existing three launches (yv3_augment_images + yv3_augment_labels, 416 x 416) on the same sources, for scale
  loader         TrainBatches over a temporary list of 64 640x480 JPEGs, bs 16, every source resident: ms per batch of whole
                 epochs with extra=False and extra=True, interleaved (--loader)
Device events around each, median of --rounds interleaved rounds after warm-up.  Bytes moved: every step reads and writes the
batch once (halo re-reads come from cache and are not counted).  One JSON line per row.

    python tools/extra_augment_bench.py [--rounds 9] [--warmup 3] [--loader]
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

from yolo_v3_amd import _ffi                        # noqa: E402
from yolo_v3_amd import augment as aug              # noqa: E402
from yolo_v3_amd import extra_augment as extra      # noqa: E402

H, W = 480, 640
KEY = 0x9E3779B97F4A7C15
ROWS = [("gauss sigma 3.0", [("GAUSS", 3.0)]), ("average k 7", [("AVERAGE", 7)]), ("median k 11", [("MEDIAN", 11)]),
        ("median k 3", [("MEDIAN", 3)]), ("sharpen", [("SHARPEN", 0.5, 1.5)]), ("noise per channel", [("NOISE", 12.75, True, KEY)]),
        ("noise per pixel", [("NOISE", 12.75, False, KEY)]), ("add", [("ADD", 5, -5, 3)]), ("mul", [("MUL", 0.8, 1.2, 1.1)]),
        ("contrast", [("CONTRAST", 0.5, 2.0, 1.5)]), ("copy", [])]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def upload_programs(programs):
    return torch.from_numpy(extra.pack_programs(programs).view(np.uint8).reshape(-1).copy()).cuda()


def setup(bs):
    rng = np.random.RandomState(bs)
    # natural-image-like sources (smooth ramps plus noise): the median's counting rounds do not depend on content, nothing else does either
    imgs = []
    for i in range(bs):
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), ((xx + yy + 31 * i) * 97 // 64) % 256], -1)
        imgs.append(np.clip(base + rng.randint(-30, 31, (H, W, 3)), 0, 255).astype(np.uint8))
    n = H * W * 3
    offs = [i * n for i in range(bs)]
    sampled = extra.sample_extra(range(bs), [(H, W)] * bs)
    d = dict(src=torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).cuda(), bytes=bs * n,
             offsets=torch.tensor(offs, dtype=torch.int64, device="cuda"),
             hw=torch.tensor([[H, W]] * bs, dtype=torch.int32, device="cuda"),
             out=torch.empty(bs * n, dtype=torch.uint8, device="cuda"), ws=torch.empty(bs * n, dtype=torch.uint8, device="cuda"),
             status=torch.empty(2 * bs, dtype=torch.int32, device="cuda"),
             programs={name: upload_programs([prog] * bs) for name, prog in ROWS},
             params=torch.from_numpy(aug.sample_params(np.arange(bs), shapes=[(H, W)] * bs)).cuda(),
             labels=torch.zeros((bs, 20, 5), dtype=torch.float64, device="cuda"),
             x=torch.empty((bs, 3, 416, 416), device="cuda"), target=torch.empty((bs, 90, 5), device="cuda"))
    d["programs"]["sampled"] = upload_programs(sampled)
    return imgs, sampled, d


def run_extra(d, bs, name):
    lib = _ffi.lib()
    _ffi.check(lib.yv3_extra_augment(d["src"].data_ptr(), d["bytes"], d["offsets"].data_ptr(), d["hw"].data_ptr(),
                                     d["programs"][name].data_ptr(), bs, d["out"].data_ptr(), d["bytes"], d["offsets"].data_ptr(),
                                     d["ws"].data_ptr(), d["bytes"], d["status"].data_ptr(), _ffi.stream_ptr()))


def run_augment(d, bs):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    _ffi.check(lib.yv3_augment_images(d["src"].data_ptr(), d["bytes"], d["offsets"].data_ptr(), d["hw"].data_ptr(),
                                      d["params"].data_ptr(), bs, d["x"].data_ptr(), 416, 416, d["ws"].data_ptr(), d["bytes"],
                                      d["status"].data_ptr(), s))
    _ffi.check(lib.yv3_augment_labels(d["labels"].data_ptr(), bs, 20, d["hw"].data_ptr(), d["params"].data_ptr(),
                                      d["target"].data_ptr(), 90, 416, 416, d["status"].data_ptr() + 4 * bs, s))


def loader_ms(bs, n_batches, rounds, root):
    """ms per batch of whole resident epochs, extra off and on: median (min, max) of `rounds` interleaved epochs each."""
    lst = os.path.join(root, "train.txt")
    full = aug.TrainBatches(lst, bs, (416, 416), seed=1).decoded_bytes()
    loaders = {on: aug.TrainBatches(lst, bs, (416, 416), seed=1, cache_bytes=full, extra=on) for on in (False, True)}
    times = {False: [], True: []}
    for r in range(rounds + 2):                            # the first epoch decodes and admits every source, the second warms up
        for on, loader in loaders.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for x, target in loader:
                pass
            torch.cuda.synchronize()
            if r >= 2:
                times[on].append((time.perf_counter() - t) * 1e3 / n_batches)
    return {on: (float(np.median(v)), min(v), max(v)) for on, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loader", action="store_true")
    a = ap.parse_args()
    sizes = (16, 64)
    state = {bs: setup(bs) for bs in sizes}
    names = [name for name, _ in ROWS] + ["sampled"]
    times = {(bs, n): [] for bs in sizes for n in names + ["end to end", "augment"]}
    for r in range(a.warmup + a.rounds):
        for bs in sizes:                                   # interleaved: every row once per round
            imgs, sampled, d = state[bs]
            row = {n: event_ms(lambda: run_extra(d, bs, n)) for n in names}
            row["end to end"] = event_ms(lambda: extra.extra_augment_batch(imgs, sampled))
            row["augment"] = event_ms(lambda: run_augment(d, bs))
            if r >= a.warmup:
                for n, t in row.items():
                    times[(bs, n)].append(t)
    for bs in sizes:
        batch = bs * H * W * 3
        steps = {name: max(len(prog), 1) for name, prog in ROWS}
        steps["sampled"] = steps["end to end"] = sum(max(len(p), 1) for p in state[bs][1]) / bs
        for n in names + ["end to end", "augment"]:
            ms = float(np.median(times[(bs, n)]))
            line = {"bs": bs, "src": "640x480", "row": n, "ms": round(ms, 4), "min_ms": round(min(times[(bs, n)]), 4),
                    "max_ms": round(max(times[(bs, n)]), 4), "rounds": a.rounds}
            if n in steps:
                moved = int(2 * batch * steps[n])
                line.update(steps_per_image=round(steps[n], 3), bytes_moved=moved, GBps=round(moved / ms / 1e6, 1))
            print(json.dumps(line))
    if a.loader:
        from PIL import Image
        with tempfile.TemporaryDirectory() as root:
            os.mkdir(os.path.join(root, "images"))
            paths = []
            for i, im in enumerate(state[64][0]):
                paths.append(os.path.join(root, "images", "s%d.jpg" % i))
                Image.fromarray(im).save(paths[-1], format="JPEG", quality=90)
            with open(os.path.join(root, "train.txt"), "w") as f:
                f.write("\n".join(paths) + "\n")
            for extra_on, (med, lo, hi) in loader_ms(16, 4, a.rounds, root).items():
                print(json.dumps({"row": "loader, resident sources, bs 16, 416", "extra": extra_on, "ms_per_batch": round(med, 3),
                                  "min": round(lo, 3), "max": round(hi, 3), "rounds": a.rounds}))


if __name__ == "__main__":
    main()
