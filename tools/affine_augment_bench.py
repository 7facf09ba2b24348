"""Time the affine augmentation on the GPU (yolo_v3_amd/affine_augment.py, csrc/affine_augment.hip): 640x480 sources, bs 16
and 64.

  inactive       yv3_affine_augment with every image inactive: the kernel's copy
  identity       every image active under the identity (every output pixel interpolates, none is padded)
  sampled        the programs sample_affine draws for seeds 0 .. bs-1 at its defaults (about half the images active)
  45 deg x 1.5   every image rotated by 45 degrees and zoomed by 1.5
  labels         yv3_affine_labels on 20 rows per image under the sampled programs
  end to end     affine_augment_batch from host numpy images and label lists with the sampled programs: packing, the one upload,
                 both launches
  extras' copy   yv3_extra_augment on programs without steps (tools/extra_augment_bench.py's "copy" row), which moves the same
                 bytes: the yardstick, measured in the same rounds
  loader         TrainBatches over a temporary list of 64 640x480 JPEGs with five boxes each, bs 16, every source resident: ms per
                 batch of whole epochs with affine off and on, interleaved (--loader)
Device events around each, median of --rounds interleaved rounds after warm-up.  Bytes moved: each image read once and written
once (the bilinear taps' re-reads come from cache and are not counted).  One JSON line per row.

    python tools/affine_augment_bench.py [--rounds 9] [--warmup 3] [--loader]
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from yolo_v3_amd import _ffi                        # noqa: E402
from yolo_v3_amd import affine_augment as affine    # noqa: E402
from yolo_v3_amd import augment as aug              # noqa: E402
from yolo_v3_amd import extra_augment as extra      # noqa: E402

H, W, T = 480, 640, 20
ROWS = ["inactive", "identity", "sampled", "45 deg x 1.5"]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def upload(records):
    return torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).cuda()


def fixed(active=1, **kw):
    fwd, inv = affine.affine_matrices(H, W, **kw)
    return {"active": active, "shape": (H, W), "fwd": fwd, "inv": inv}


def setup(bs):
    rng = np.random.RandomState(bs)
    imgs = []
    for i in range(bs):                                    # natural-image-like sources: smooth ramps plus noise (no time depends on content)
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), ((xx + yy + 31 * i) * 97 // 64) % 256], -1)
        imgs.append(np.clip(base + rng.randint(-30, 31, (H, W, 3)), 0, 255).astype(np.uint8))
    n = H * W * 3
    sampled = affine.sample_affine(range(bs), [(H, W)] * bs)
    programs = {"inactive": [fixed(active=0)] * bs, "identity": [fixed()] * bs, "sampled": sampled,
                "45 deg x 1.5": [fixed(theta=math.radians(45), scale=1.5)] * bs}
    labels = np.zeros((bs, T, 5))
    labels[..., 0] = rng.randint(0, 80, (bs, T))
    labels[..., 1:3] = rng.uniform(0.1, 0.9, (bs, T, 2))
    labels[..., 3:5] = rng.uniform(0.05, 0.4, (bs, T, 2))
    d = dict(src=torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).cuda(), bytes=bs * n,
             offsets=torch.tensor([i * n for i in range(bs)], dtype=torch.int64, device="cuda"),
             hw=torch.tensor([[H, W]] * bs, dtype=torch.int32, device="cuda"),
             out=torch.empty(bs * n, dtype=torch.uint8, device="cuda"), ws=torch.empty(bs * n, dtype=torch.uint8, device="cuda"),
             status=torch.empty(2 * bs, dtype=torch.int32, device="cuda"),
             programs={name: upload(affine.pack_programs(p)) for name, p in programs.items()},
             no_steps=upload(extra.pack_programs([[]] * bs)),
             labels=torch.from_numpy(labels).cuda(), labels_out=torch.empty((bs, T, 5), dtype=torch.float64, device="cuda"))
    return imgs, [l for l in labels], sampled, d


def run_pixels(d, bs, name):
    _ffi.check(_ffi.lib().yv3_affine_augment(d["src"].data_ptr(), d["bytes"], d["offsets"].data_ptr(), d["hw"].data_ptr(),
                                             d["programs"][name].data_ptr(), bs, d["out"].data_ptr(), d["bytes"],
                                             d["offsets"].data_ptr(), d["status"].data_ptr(), _ffi.stream_ptr()))


def run_labels(d, bs):
    _ffi.check(_ffi.lib().yv3_affine_labels(d["labels"].data_ptr(), bs, T, d["hw"].data_ptr(), d["programs"]["sampled"].data_ptr(),
                                            d["labels_out"].data_ptr(), d["status"].data_ptr() + 4 * bs, _ffi.stream_ptr()))


def run_extras_copy(d, bs):
    _ffi.check(_ffi.lib().yv3_extra_augment(d["src"].data_ptr(), d["bytes"], d["offsets"].data_ptr(), d["hw"].data_ptr(),
                                            d["no_steps"].data_ptr(), bs, d["out"].data_ptr(), d["bytes"], d["offsets"].data_ptr(),
                                            d["ws"].data_ptr(), d["bytes"], d["status"].data_ptr(), _ffi.stream_ptr()))


def loader_ms(bs, n_batches, rounds, root):
    """ms per batch of whole resident epochs, affine off and on: median (min, max) of `rounds` interleaved epochs each."""
    lst = os.path.join(root, "train.txt")
    full = aug.TrainBatches(lst, bs, (416, 416), seed=1).decoded_bytes()
    loaders = {on: aug.TrainBatches(lst, bs, (416, 416), seed=1, cache_bytes=full, affine=on) for on in (False, True)}
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
    names = ROWS + ["labels", "end to end", "extras' copy"]
    times = {(bs, n): [] for bs in sizes for n in names}
    for r in range(a.warmup + a.rounds):
        for bs in sizes:                                   # interleaved: every row once per round
            imgs, labels, sampled, d = state[bs]
            row = {n: event_ms(lambda: run_pixels(d, bs, n)) for n in ROWS}
            row["labels"] = event_ms(lambda: run_labels(d, bs))
            row["end to end"] = event_ms(lambda: affine.affine_augment_batch(imgs, labels, sampled))
            row["extras' copy"] = event_ms(lambda: run_extras_copy(d, bs))
            if r >= a.warmup:
                for n, t in row.items():
                    times[(bs, n)].append(t)
    for bs in sizes:
        moved = 2 * bs * H * W * 3
        for n in names:
            ms = float(np.median(times[(bs, n)]))
            line = {"bs": bs, "src": "640x480", "row": n, "ms": round(ms, 4), "min_ms": round(min(times[(bs, n)]), 4),
                    "max_ms": round(max(times[(bs, n)]), 4), "rounds": a.rounds}
            if n == "sampled" or n == "end to end":
                line["active"] = sum(p["active"] for p in state[bs][2])
            if n != "labels":
                line.update(bytes_moved=moved, GBps=round(moved / ms / 1e6, 1))
            print(json.dumps(line))
    if a.loader:
        from PIL import Image
        with tempfile.TemporaryDirectory() as root:
            os.mkdir(os.path.join(root, "images"))
            os.mkdir(os.path.join(root, "labels"))
            paths = []
            for i, im in enumerate(state[64][0]):
                paths.append(os.path.join(root, "images", "s%d.jpg" % i))
                Image.fromarray(im).save(paths[-1], format="JPEG", quality=90)
                np.savetxt(aug.label_path(paths[-1]), state[64][1][i][:5])
            with open(os.path.join(root, "train.txt"), "w") as f:
                f.write("\n".join(paths) + "\n")
            for on, (med, lo, hi) in loader_ms(16, 4, a.rounds, root).items():
                print(json.dumps({"row": "loader, resident sources, bs 16, 416", "affine": on, "ms_per_batch": round(med, 3),
                                  "min": round(lo, 3), "max": round(hi, 3), "rounds": a.rounds}))


if __name__ == "__main__":
    main()
