"""Time the training augmentation (yolo_v3_amd/augment.py, csrc/augment.hip): 640x480 sources to 416 and 608, bs 16 and 64.

  kernels     the three launches alone (yv3_augment_images + yv3_augment_labels on sources already on the device)
  end to end  augment_batch from host numpy images: packing into pinned memory, the one upload, the launches
Device events around each, median of --rounds interleaved rounds after warm-up.  Also printed: the bytes the kernels move (sources
read, colour copy written and read back by the resample, fp32 batch written; taps re-read from cache not counted) and the rate
they imply.  One JSON line per configuration.

    python tools/augment_bench.py [--rounds 9] [--warmup 3] [--labels 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from yolo_v3_amd import _ffi                  # noqa: E402
from yolo_v3_amd import augment as aug        # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def setup(bs, dim, n_labels):
    rng = np.random.RandomState(bs + dim)
    imgs = [rng.randint(0, 256, (480, 640, 3)).astype(np.uint8) for _ in range(bs)]
    labels = []
    for _ in range(bs):
        r = np.zeros((n_labels, 5))
        r[:, 0] = rng.randint(0, 80, n_labels)
        r[:, 1:] = rng.uniform(0.1, 0.6, (n_labels, 4))
        labels.append(r)
    params = aug.sample_params(np.arange(bs), shapes=imgs)
    # device-resident copy of what augment_batch uploads, for the kernel-only timing
    offs, pos = [], 0
    for im in imgs:
        offs.append(pos)
        pos += im.size
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).cuda()
    dev = dict(src=src, src_bytes=pos, offsets=torch.tensor(offs, dtype=torch.int64, device="cuda"),
               hw=torch.tensor([im.shape[:2] for im in imgs], dtype=torch.int32, device="cuda"),
               params=torch.from_numpy(params).cuda(), labels=torch.from_numpy(np.stack(labels)).cuda(),
               x=torch.empty((bs, 3, dim, dim), device="cuda"), target=torch.empty((bs, 90, 5), device="cuda"),
               ws=torch.empty(pos, dtype=torch.uint8, device="cuda"), status=torch.empty(2 * bs, dtype=torch.int32, device="cuda"))
    return imgs, labels, params, dev


def kernels(d, bs, dim, n_labels):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    _ffi.check(lib.yv3_augment_images(d["src"].data_ptr(), d["src_bytes"], d["offsets"].data_ptr(), d["hw"].data_ptr(),
                                      d["params"].data_ptr(), bs, d["x"].data_ptr(), dim, dim, d["ws"].data_ptr(), d["ws"].numel(),
                                      d["status"].data_ptr(), s))
    _ffi.check(lib.yv3_augment_labels(d["labels"].data_ptr(), bs, n_labels, d["hw"].data_ptr(), d["params"].data_ptr(),
                                      d["target"].data_ptr(), 90, dim, dim, d["status"].data_ptr() + 4 * bs, s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--labels", type=int, default=20)
    a = ap.parse_args()
    configs = [(bs, dim) for bs in (16, 64) for dim in (416, 608)]
    state = {c: setup(c[0], c[1], a.labels) for c in configs}
    times = {c: {"kernels": [], "end_to_end": []} for c in configs}
    for r in range(a.warmup + a.rounds):
        for c in configs:                                  # interleaved: every configuration once per round
            bs, dim = c
            imgs, labels, params, d = state[c]
            tk = event_ms(lambda: kernels(d, bs, dim, a.labels))
            te = event_ms(lambda: aug.augment_batch(imgs, labels, (dim, dim), params))
            if r >= a.warmup:
                times[c]["kernels"].append(tk)
                times[c]["end_to_end"].append(te)
    for c in configs:
        bs, dim = c
        src = bs * 480 * 640 * 3
        moved = src + 2 * src + bs * 3 * dim * dim * 4              # read sources; write + read the colour copy; write the batch
        k = float(np.median(times[c]["kernels"]))
        e = float(np.median(times[c]["end_to_end"]))
        print(json.dumps({"bs": bs, "dim": dim, "src": "640x480", "kernels_ms": round(k, 4), "end_to_end_ms": round(e, 4),
                          "upload_bytes": src, "kernel_bytes": moved, "kernel_GBps": round(moved / k / 1e6, 1),
                          "kernels_min_ms": round(min(times[c]["kernels"]), 4), "end_to_end_min_ms": round(min(times[c]["end_to_end"]), 4),
                          "end_to_end_max_ms": round(max(times[c]["end_to_end"]), 4),
                          "rounds": a.rounds}))


if __name__ == "__main__":
    main()
