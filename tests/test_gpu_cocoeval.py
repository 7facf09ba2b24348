"""COCO bbox evaluation on the MI355X (csrc/cocoeval.hip through yolo_v3_amd.cocoeval) against the float64 restatement
(tests/cocoeval_np.py): every precision / recall / scores array bit-identical, stats identical."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from tests import cocoeval_np
from yolo_v3_amd import _ffi, synth
from yolo_v3_amd.cocoeval import COCO, COCOeval, evaluate_detections, detections_as_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)


def _gpu_eval(gt, res, imgIds=None, iouThrs=None, maxDets=None):
    cg = COCO(gt)
    cd = cg.loadRes(res)
    e = COCOeval(cg, cd, 'bbox')
    if imgIds is not None:
        e.params.imgIds = imgIds
    if iouThrs is not None:
        e.params.iouThrs = np.asarray(iouThrs, dtype=np.float64)
    if maxDets is not None:
        e.params.maxDets = maxDets
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        e.evaluate()
        e.accumulate()
        e.summarize()
    return e, out.getvalue()


def _assert_same(e, ref):
    for k in ("precision", "recall", "scores"):
        assert e.eval[k].shape == ref[k].shape, k
        bad = np.argwhere(e.eval[k] != ref[k])
        assert bad.size == 0, "%s differs at %d entries, first %s: gpu %r restatement %r" % (
            k, len(bad), tuple(bad[0]), e.eval[k][tuple(bad[0])], ref[k][tuple(bad[0])])
    assert np.array_equal(e.stats, ref["stats"])


def test_notebook_toy_case(golden_dir):
    nb = json.load(open(os.path.join(golden_dir, "cocoeval_notebook.json")))
    e, printed = _gpu_eval(nb["gt"], nb["results"], imgIds=nb["imgIds"])
    assert [ln for ln in printed.splitlines() if ln.startswith(" Average")] == nb["printed"]
    assert [round(float(s), 3) for s in e.stats] == nb["stats"]
    _assert_same(e, cocoeval_np.evaluate(nb["gt"], nb["results"], imgIds=nb["imgIds"]))


# (seed, options): together they cover crowd GTs, a GT with id 0, score ties inside and across images, a group with more than
# 100 dets, areas exactly 32^2 / 96^2, zero-width boxes, categories with dets but no GT, images with GT but no dets (every set),
# an imgIds subset, non-default iouThrs and maxDets.
CASES = [(s, {}) for s in range(1, 9)] + [
    (11, {"id0": True}), (12, {"id0": True, "big_group": True}), (13, {"big_group": True}), (14, {"crowd": False}),
    (15, {"subset": True}), (16, {"subset": True, "id0": True}), (17, {"iou": [0.1, 0.3, 0.5, 0.7, 0.9, 0.99]}),
    (18, {"maxDets": [5, 20, 120]}), (19, {"maxDets": [100, 1, 10], "big_group": True}),
    (20, {"iou": [0.5, 0.75], "maxDets": [2, 3, 4]}), (21, {"n_img": 60, "gt_per_img": 20, "det_per_img": 60}),
    (22, {"n_cat": 3, "det_per_img": 40}),
]


@pytest.mark.parametrize("seed,opt", CASES, ids=["s%d" % s for s, _ in CASES])
def test_synthetic_sets_match_restatement(seed, opt):
    opt = dict(opt)
    subset, iou, md = opt.pop("subset", False), opt.pop("iou", None), opt.pop("maxDets", None)
    gt, res = cocoeval_np.synthetic_set(seed, **opt)
    imgIds = [im["id"] for im in gt["images"]][1::2] if subset else None
    e, _ = _gpu_eval(gt, res, imgIds=imgIds, iouThrs=iou, maxDets=md)
    ref = cocoeval_np.evaluate(gt, res, imgIds=imgIds, iouThrs=iou, maxDets=md)
    _assert_same(e, ref)


def test_large_set_matches_restatement_and_is_deterministic():
    gt, res = cocoeval_np.synthetic_set(7, n_img=500, n_cat=80, gt_per_img=14, det_per_img=200)
    assert len(res) > 35000
    e1, _ = _gpu_eval(gt, res)
    e2, _ = _gpu_eval(gt, res)
    for k in ("precision", "recall", "scores"):
        assert np.array_equal(e1.eval[k], e2.eval[k])
        assert e1.eval[k].tobytes() == e2.eval[k].tobytes()
    _assert_same(e1, cocoeval_np.evaluate(gt, res))


def test_group_over_the_gt_limit_raises():
    gt = {"images": [{"id": 1}], "categories": [{"id": 0}],
          "annotations": [{"id": i + 1, "image_id": 1, "category_id": 0, "iscrowd": 0, "area": 100.0,
                           "bbox": [float(i), 0.0, 10.0, 10.0]} for i in range(257)]}
    res = [{"image_id": 1, "category_id": 0, "bbox": [0.0, 0.0, 10.0, 10.0], "score": 0.5}]
    with pytest.raises(_ffi.Yv3Error, match="limit"):
        _gpu_eval(gt, res)
    gt["annotations"] = gt["annotations"][:256]                  # at the limit: fine
    e, _ = _gpu_eval(gt, res)
    _assert_same(e, cocoeval_np.evaluate(gt, res))


def test_maxdets_over_the_limit_raises():
    gt, res = cocoeval_np.synthetic_set(3)
    with pytest.raises(_ffi.Yv3Error, match="limit"):
        _gpu_eval(gt, res, maxDets=[1, 10, 2000])


def _as_coco(arrays, n_img, n_cat):
    """The arrays of detections_as_arrays as a COCO ground truth + results pair (for the restatement)."""
    gt = {"images": [{"id": i} for i in range(n_img)], "categories": [{"id": c} for c in range(n_cat)],
          "annotations": [{"id": int(arrays["gt_id"][j]), "image_id": int(arrays["gt_img"][j]), "category_id": int(arrays["gt_cat"][j]),
                           "iscrowd": 0, "area": float(arrays["gt_area"][j]), "bbox": [float(v) for v in arrays["gt_box"][j]]}
                          for j in range(len(arrays["gt_id"]))]}
    res = [{"image_id": int(arrays["det_img"][j]), "category_id": int(arrays["det_cat"][j]),
            "bbox": [float(v) for v in arrays["det_box"][j]], "score": float(arrays["det_score"][j])}
           for j in range(len(arrays["det_img"]))]
    return gt, res


def test_end_to_end_modes_against_f32_pseudo_ground_truth(sw1_stream, tmp_path):
    """F32 detections at conf >= 0.5 are the pseudo ground truth, written by the annotations writer from darknet label files;
    scoring the same detections gives AP 1.0 wherever AP is defined -- to pycocotools' epsilon: precision tp / (tp + fp + 2^-52)
    is 1 - 2^-52 when tp = 1 (after renumbering the ids from 1: the first annotation
    has id 0, which COCOeval never counts as found); F32H2 / BF16 detections scored against it equal the restatement."""
    from PIL import Image
    from tests.helpers import load_sw1_net
    from yolo_v3_amd import detect, evaluate
    net = load_sw1_net(sw1_stream).cuda()
    x = torch.from_numpy(synth.images(4, 416, 4242)).cuda()
    net.math_mode = _ffi.F32
    ref = detect(net, x, obj_conf_thr=0.5)
    assert sum(len(r) for r in ref) > 0
    (tmp_path / "images").mkdir()
    (tmp_path / "labels").mkdir()
    paths = []
    for i, r in enumerate(ref):
        p = str(tmp_path / "images" / ("scene_%06d.jpg" % (i + 1)))
        Image.new("RGB", (416, 416)).save(p)
        rows = []
        for b in (r.cpu().double().numpy() if len(r) else np.zeros((0, 7))):
            w, h = b[2] - b[0], b[3] - b[1]
            rows.append("%d %.17g %.17g %.17g %.17g" % (int(b[6]), (b[0] + w / 2) / 416, (b[1] + h / 2) / 416, w / 416, h / 416))
        with open(p.replace("jpg", "txt").replace("images", "labels"), "w") as f:
            f.write("\n".join(rows) + ("\n" if rows else ""))
        paths.append(p)
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    gt = evaluate.create_annotations_dict(str(tmp_path / "list.txt"), ["c%d" % c for c in range(80)])
    assert gt["annotations"][0]["id"] == 0
    res = [{"image_id": i + 1, "category_id": int(b[6]), "score": float(b[5]),
            "bbox": [float(b[0]), float(b[1]), float(b[2]) - float(b[0]), float(b[3]) - float(b[1])]}
           for i, r in enumerate(ref) for b in r.cpu().numpy()]
    for a in gt["annotations"]:
        a["id"] += 1
    # random weights put many boxes of one class in one image: keep every one of them (maxDets[-1] = the largest group)
    sizes = {}
    for r in res:
        sizes[r["image_id"], r["category_id"]] = sizes.get((r["image_id"], r["category_id"]), 0) + 1
    big = max(100, max(sizes.values()))
    assert big <= 1024
    e, _ = _gpu_eval(gt, res, maxDets=[1, 10, big])
    at_all = e.eval["precision"][..., -1]
    one = 1.0 / (1.0 + np.spacing(1))        # pr = tp / (tp + fp + eps) of a category whose only box is found: 1 - 2^-52
    bad = np.argwhere((at_all > -1) & (at_all != 1.0) & (at_all != one))
    assert bad.size == 0, "AP < 1 at %d entries (t, r, k, a) e.g. %s = %r; recall %r; largest group %d" % (
        len(bad), tuple(bad[0]), at_all[tuple(bad[0])], e.eval["recall"][bad[0][0], bad[0][2], bad[0][3], -1], big)
    assert (at_all > -1).any()
    _assert_same(e, cocoeval_np.evaluate(gt, res, maxDets=[1, 10, big]))
    # the modes, through the tensor-level entry point
    for mode in (_ffi.F32H2, _ffi.BF16):
        net.math_mode = mode
        got = detect(net, x, obj_conf_thr=0.3)
        ev = evaluate_detections(got, ref, num_classes=80)
        g2, r2 = _as_coco(detections_as_arrays(got, ref), len(ref), 80)
        want = cocoeval_np.evaluate(g2, r2)
        for k in ("precision", "recall", "scores"):
            assert np.array_equal(ev[k], want[k]), (mode, k)
        assert np.array_equal(ev["stats"], want["stats"])
    net.math_mode = _ffi.F32
