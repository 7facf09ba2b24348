"""Write tests/golden/yolo_loss.npz: the reference's YoloLayer.forward(x, img_dim, target) 10-tuple and x.grad on the cases of
tests/yolo_loss_ref.CASES, computed by the reference's own yololayer.py on the CPU (the shims of oracle.make_golden.import_reference).

Each case's inputs are regenerated from yolo_v3_amd.synth seeds (tests/yolo_loss_ref.make_case); a random draw in which an IoU lies
within 1e-4 of 0.5 or 0.7, two anchors' IoUs within 1e-4 of each other, or a GT centre within 1e-4 of a cell border is re-drawn
(`attempt`, stored with the case), so that no decision is left to the last ulp.

    python tools/make_golden_yolo_loss.py [out.npz]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle.make_golden import import_reference          # noqa: E402
from tests import yolo_loss_ref as R                     # noqa: E402


def main(out):
    torch, _, yololayer, _, _ = import_reference()
    arrays = {}
    for spec in R.CASES:
        for attempt in range(200):
            x, tg = R.make_case(spec, attempt)
            res = R.yolo_loss(x, tg, R.ANCHORS, spec["mask"], spec["img_dim"][1], spec["C"])
            if R.margins_ok(res["margins"]):
                break
        else:
            raise RuntimeError("no draw of %s clears the margins" % spec["name"])
        layer = yololayer.YoloLayer(R.ANCHORS, spec["mask"], spec["img_dim"], spec["C"])
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        out_t = layer(xt, spec["img_dim"], torch.from_numpy(tg))
        out_t[0].backward()
        vals = np.array([float(out_t[0].item())] + [float(v) for v in out_t[1:8]], np.float64)
        n = spec["name"]
        arrays[n + "/attempt"] = np.array(attempt)
        arrays[n + "/values"] = vals                      # loss, loss/nB, loss_x/nB .. loss_cls/nB
        arrays[n + "/counts"] = np.array([int(out_t[8]), int(out_t[9])], np.int64)
        arrays[n + "/grad"] = xt.grad.numpy().astype(np.float32)
        print("%-14s attempt %d  loss %.6g  nCorrect %d  nGT %d  margins %s" % (n, attempt, vals[0], out_t[8], out_t[9],
                                                                             {k: round(v, 5) for k, v in res["margins"].items()}))
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "yolo_loss.npz"))
