"""A/B of math modes on one GPU in one process: `Detector` (network + post-processing) in two or more modes, rounds interleaved after a
warm-up, timed with device events; prints the median and range of images/s per mode and the ratio to the first mode.

    python tools/mode_ab.py --modes BF16,F16 --size 416 --batch 64 --rounds 9 [--steps 8] [--warmup 3] [--accuracy]

--accuracy adds, per mode, the relative L2 error of the three heads' logits against the fp32 oracle (CPU) on two images and the boxes
line (oracle.boxdelta at IOU >= 0.5) of `detect` against the oracle's boxes.  I8 is calibrated on the timed batch before anything is timed
(and, for --accuracy, on the two accuracy images)."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from yolo_v3_amd import _ffi, synth, Detector, YoloNet, WeightManager, detect          # noqa: E402

MODES = {"F32": _ffi.F32, "BF16": _ffi.BF16, "F32X3": _ffi.F32X3, "F32H2": _ffi.F32H2, "F16": _ffi.F16, "I8": _ffi.I8}


def load_net(size):
    stream = synth.weight_stream()
    net = YoloNet((size, size)).eval()
    assert WeightManager(net).load_stream(stream) == stream.size
    return net.cuda(), stream


def time_round(det, x, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        det.run_device(x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps                       # ms per batch


def accuracy(net, stream, names):
    from oracle import oracle_cpu as oc
    from oracle.boxdelta import boxes_delta
    sd, _ = oc.state_dict_from_stream(stream)
    x = torch.from_numpy(synth.images(2, 416, 2007))
    with torch.no_grad():
        ref = oc.head_logits(sd, x)
        want = oc.postprocess(torch.cat(oc.yolonet_forward(sd, x), 1), 80, 0.5, 0.4)
    out, asked = {}, net.math_mode
    if "I8" in names:
        net.calibrate_int8([x.cuda()])
    for name in names:
        mode = MODES[name]
        with torch.no_grad():
            _, plan = net.engine(mode).forward(x.cuda(), logits=True)
        torch.cuda.synchronize()
        errs = [float((lg.permute(0, 3, 1, 2).cpu().double() - r.double()).norm() / r.double().norm()) for (lg, _, _), r in zip(plan.logits, ref)]
        net.math_mode = mode
        d = boxes_delta(detect(net, x.cuda()), want, 2, iou_match=0.5)
        out[name] = {"logits_rel_l2": [float("%.4g" % e) for e in errs],
                     "boxes": {k: d[k] for k in ("ref_boxes", "got_boxes", "matched", "unmatched_ref", "unmatched_got", "unmatched_frac")}}
    net.math_mode = asked
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="BF16,F16")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=None)
    ap.add_argument("--accuracy", action="store_true")
    args = ap.parse_args()
    names = [m.strip().upper() for m in args.modes.split(",") if m.strip()]
    assert len(names) >= 2 and all(n in MODES for n in names), "modes: two or more of %s" % ", ".join(MODES)
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.set_device(0)
    net, stream = load_net(args.size)
    x = torch.from_numpy(synth.images(args.batch, args.size, 7)).cuda()
    if "I8" in names:
        net.calibrate_int8([x])
    dets = {n: Detector(net, args.batch, args.size, args.size, 0.5, 0.4, dtype=MODES[n], lanes=args.lanes) for n in names}
    with torch.no_grad():
        for n in names:
            for _ in range(args.warmup):
                dets[n](x)
            assert dets[n].engine.dtype == MODES[n], "%s fell back to mode %d" % (n, dets[n].engine.dtype)
        ms = {n: [] for n in names}
        for r in range(args.rounds):
            for n in (names if r % 2 == 0 else names[::-1]):          # interleaved, order alternating
                ms[n].append(time_round(dets[n], x, args.steps))
    res = {"size": args.size, "batch": args.batch, "rounds": args.rounds, "steps": args.steps, "modes": {}}
    for n in names:
        ips = sorted(args.batch / (t / 1e3) for t in ms[n])
        res["modes"][n] = {"lanes": dets[n].lanes, "images_per_s_median": round(statistics.median(ips), 1),
                           "images_per_s_min": round(ips[0], 1), "images_per_s_max": round(ips[-1], 1)}
    base = res["modes"][names[0]]["images_per_s_median"]
    for n in names[1:]:
        res["modes"][n]["ratio_to_" + names[0]] = round(res["modes"][n]["images_per_s_median"] / base, 4)
    if args.accuracy:
        res["accuracy"] = accuracy(load_net(416)[0] if args.size != 416 else net, stream, names)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
