"""Write tests/golden/train_step.npz: one training step of the reference's own YoloNet (darknet.py, yololayer.py) on the CPU, in
.train() and in .eval(): `loss = net(x, target); loss.backward()` (the shims of oracle.make_golden.import_reference).

The case (tests/test_train_host.CASE): 96x96, bs=2, 3 classes, tests/helpers.trained_like_stream weights, yolo_v3_amd.synth images.
The target rows are the first seeded draw whose decisions (IoU against 0.5 / 0.7, best anchor, cell) all clear the 1e-4 margins on
the float64 restatement's logits (tests/train_ref.py), as tools/make_golden_yolo_loss.py does for the loss alone.  Stored per mode:
the loss and the 9 stats, the running statistics after the .train() step (as their change), the full gradients of every BatchNorm
weight / bias and head bias, and for each conv weight the gradient's fp64 sum, sum of squares and 32 seeded entries.  The full
tensors are stored as fp16 with a power-of-two scale per tensor (tests/test_train_host.put16): 2^-11 relative per element, which
keeps the file near 0.3 MB.

    python tools/make_golden_train.py [out.npz]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle.make_golden import import_reference          # noqa: E402
from tests import test_train_host as H                   # noqa: E402


def main(out):
    torch, darknet, _, _, _ = import_reference()
    sd, x, tg, attempt = H.case()
    arrays = {"target": tg, "attempt": np.array(attempt)}
    for mode in ("train", "eval"):
        torch.manual_seed(0)
        net = darknet.YoloNet((H.CASE["size"], H.CASE["size"]), numClass=H.CASE["C"])
        net.load_state_dict(sd)
        net.train(mode == "train")
        loss = net(torch.from_numpy(x.copy()), torch.from_numpy(tg.copy()))
        loss.backward()
        st = net.stats
        arrays[mode + "/loss"] = np.array(float(loss.item()), np.float64)
        arrays[mode + "/stats"] = np.array([float(st[k]) for k in net.stat_keys[:9]], np.float64)   # loss/B .. nGT
        if mode == "train":                               # (.eval() leaves them as they were)
            nsd = net.state_dict()
            H.put16(arrays, "train/running_delta", [nsd[k].numpy().astype(np.float64) - sd[k].numpy().astype(np.float64)
                                                    for k in H.running_keys(sd)])
        sums, ents, vec = [], [], []
        for k, p in net.named_parameters():           # (state_dict order, as train_ref.param_names)
            g = p.grad.numpy().astype(np.float32)
            if g.ndim == 4:
                g64 = g.astype(np.float64).ravel()
                sums.append([g64.sum(), (g64 * g64).sum()])
                ents.append(g64[H.entries(k, g64.size)].astype(np.float32))
            else:
                vec.append(g)
        arrays[mode + "/conv_sums"] = np.array(sums, np.float64)
        arrays[mode + "/conv_entries"] = np.array(ents, np.float32)
        H.put16(arrays, mode + "/vec_grads", vec)
        print(mode, "loss %.6g" % float(loss.item()), {k: round(float(st[k]), 5) for k in net.stat_keys})
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes; target attempt", attempt)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "train_step.npz"))
