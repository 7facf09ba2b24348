"""Accuracy of the reduced-precision math modes at the level detection people compare: COCO AP / AR (yolo_v3_amd.cocoeval)
of F32H2, F32X3 and BF16 detections against the exact-F32 detections of the same synthetic scenes as pseudo ground truth.

SW-1 synthetic weights (no trained weights ship), synth.images scenes; pseudo-GT = F32 detections at conf >= --gt-conf, scored
detections at conf >= --conf.  F32 against itself is printed as the ceiling.  One JSON line per mode, then the summary table.

    python tools/mode_map.py [--images 32] [--size 416] [--conf 0.3] [--gt-conf 0.5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--conf", type=float, default=0.3)
    ap.add_argument("--gt-conf", type=float, default=0.5)
    args = ap.parse_args()
    import torch
    from yolo_v3_amd import YoloNet, WeightManager, synth, detect, _ffi
    from yolo_v3_amd.cocoeval import evaluate_detections
    torch.cuda.set_device(0)
    stream = synth.weight_stream()
    net = YoloNet((args.size, args.size)).eval()
    WeightManager(net).load_stream(stream)
    net = net.cuda()

    def run(mode, conf):
        net.math_mode = mode
        out = []
        for b in range(0, args.images, args.batch):
            x = torch.from_numpy(synth.images(min(args.batch, args.images - b), args.size, 9000 + b)).cuda()
            out += [r.cpu() for r in detect(net, x, obj_conf_thr=conf)]
        return out

    gt = run(_ffi.F32, args.gt_conf)
    rows = {}
    for name, mode in (("F32", _ffi.F32), ("F32H2", _ffi.F32H2), ("F32X3", _ffi.F32X3), ("BF16", _ffi.BF16)):
        ev = evaluate_detections(run(mode, args.conf), gt, num_classes=80)
        rows[name] = [float(s) for s in ev["stats"]]
        print(json.dumps({"mode": name, "images": args.images, "gt_boxes": sum(len(g) for g in gt),
                          **{k: round(v, 4) for k, v in zip(NAMES, rows[name])}}))
    print("| mode | " + " | ".join(NAMES) + " |")
    print("|---" * (len(NAMES) + 1) + "|")
    for name, st in rows.items():
        print("| %s | " % name + " | ".join("%.3f" % s for s in st) + " |")


if __name__ == "__main__":
    main()
