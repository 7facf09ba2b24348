"""Timing of the GPU COCO bbox evaluation (yolo_v3_amd.cocoeval) on a synthetic COCO-val-sized set: 5 000 images,
80 categories, ~36 000 ground-truth boxes, ~500 000 detections (tests/cocoeval_np.synthetic_set).

Reports host JSON parse (loadRes of a results file), host id mapping, H2D copy, the device evaluation (one yv3_cocoeval
call: grouping, matching, ordering, accumulation; HIP events) and D2H, each the median of --reps runs after one warm-up;
and, for context, the float64 numpy restatement on a 500-image subset.  One JSON line on stdout.

    python tools/cocoeval_bench.py [--reps 5] [--no-restatement]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    import torch
    from tests import cocoeval_np
    from yolo_v3_amd.cocoeval import COCO, COCOeval
    torch.cuda.set_device(0)
    gt, res = cocoeval_np.synthetic_set(5000, n_img=5000, n_cat=80, gt_per_img=14, det_per_img=250)
    with tempfile.TemporaryDirectory() as tmp:
        rf = os.path.join(tmp, "res.json")
        with open(rf, "w") as f:
            json.dump(res, f)
        cg = COCO(gt)
        t0 = time.perf_counter()
        cd = cg.loadRes(rf)
        parse = time.perf_counter() - t0
    rows = []
    for i in range(args.reps + 1):
        e = COCOeval(cg, cd, 'bbox')
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            e.evaluate()
            e.accumulate()
            e.summarize()
            wall = time.perf_counter() - t0
        if i:
            rows.append(dict(e.timings, wall=wall))
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    out = {"images": 5000, "categories": 80, "gts": len(gt["annotations"]), "dets": len(res), "parse_s": parse,
           "map_s": med["map"], "h2d_s": med["h2d"], "device_s": med["device"], "d2h_s": med["d2h"],
           "evaluate_accumulate_summarize_wall_s": med["wall"], "stats": [round(float(s), 6) for s in e.stats]}
    if not args.no_restatement:
        sub = sorted(im["id"] for im in gt["images"])[:500]
        t0 = time.perf_counter()
        cocoeval_np.evaluate(gt, res, imgIds=sub)
        out["restatement_500_images_s"] = time.perf_counter() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
