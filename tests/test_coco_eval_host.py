"""COCO evaluation, host side: the ground-truth writer against the reference's bytes, the float64 restatement against the
numbers the reference notebook printed, and the COCO / COCOeval surface that needs no GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests import cocoeval_np
from yolo_v3_amd import _ffi, evaluate
from yolo_v3_amd.cocoeval import COCO, COCOeval, Params

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_images(tmp_path, inputs, skip_labels=()):
    from PIL import Image
    root = tmp_path / "coco"
    (root / "images").mkdir(parents=True)
    (root / "labels").mkdir()
    paths = []
    for i, im in enumerate(inputs["images"]):
        p = str(root / "images" / im["file"])
        Image.new("RGB", (im["width"], im["height"]), (i * 40, 90, 200)).save(p, quality=90)
        if i not in skip_labels:
            with open(p.replace("jpg", "txt").replace("images", "labels"), "w") as f:
                f.write(im["labels"])
        paths.append(p)
    target = tmp_path / "list.txt"
    target.write_text("\n".join(paths) + "\n")
    return str(target), paths


def test_annotations_file_matches_reference_bytes(golden_dir, tmp_path):
    inputs = json.load(open(os.path.join(golden_dir, "coco_gt_inputs.json")))
    target, _ = _write_images(tmp_path, inputs)
    out = tmp_path / "gt.json"
    evaluate.generate_annotations_file(target, inputs["class_names"], str(out))
    assert out.read_bytes() == open(os.path.join(golden_dir, "coco_gt_ref.json"), "rb").read()


def test_annotations_missing_label_file_means_no_annotations(golden_dir, tmp_path):
    inputs = json.load(open(os.path.join(golden_dir, "coco_gt_inputs.json")))
    target, paths = _write_images(tmp_path, inputs, skip_labels=(0, 3))
    d = evaluate.create_annotations_dict(target, inputs["class_names"])
    ref = json.load(open(os.path.join(golden_dir, "coco_gt_ref.json")))
    assert d["images"] == ref["images"]
    kept = [a for a in ref["annotations"] if a["image_id"] not in (139, 724)]
    assert [a["id"] for a in d["annotations"]] == list(range(len(kept)))
    assert [(a["image_id"], a["category_id"], a["bbox"], a["area"]) for a in d["annotations"]] == \
        [(a["image_id"], a["category_id"], a["bbox"], a["area"]) for a in kept]


def test_annotations_image_size_follows_exif_rotation(tmp_path):
    from PIL import Image
    p = tmp_path / "images" / "rot_000000000005.jpg"
    p.parent.mkdir()
    exif = Image.Exif()
    exif[0x0112] = 6                                            # rotate 90 degrees: the decoded image is 30 x 50
    Image.new("RGB", (50, 30)).save(str(p), exif=exif)
    assert evaluate.image_size(str(p)) == (30, 50)
    assert evaluate.read_image_rgb(str(p)).shape[:2] == (50, 30)
    img_list, ann_list = evaluate.get_img_ann_list([str(p)], [str(tmp_path / "none.txt")])
    assert img_list == [{"id": 5, "width": 30, "height": 50}] and ann_list == []


def _notebook(golden_dir):
    return json.load(open(os.path.join(golden_dir, "cocoeval_notebook.json")))


def test_restatement_reproduces_the_notebook(golden_dir):
    nb = _notebook(golden_dir)
    ev = cocoeval_np.evaluate(nb["gt"], nb["results"], imgIds=nb["imgIds"])
    assert [round(float(s), 3) for s in ev["stats"]] == nb["stats"]
    assert nb["stats"] == [0.667, 0.667, 0.667, -1.0, 0.667, -1.0, 0.667, 0.667, 0.667, -1.0, 0.667, -1.0]


def test_summarize_prints_the_notebook_lines(golden_dir, capsys):
    """summarize's format, on the restatement's arrays (the GPU test checks the arrays themselves)."""
    from yolo_v3_amd.cocoeval import summarize_stats
    nb = _notebook(golden_dir)
    ev = cocoeval_np.evaluate(nb["gt"], nb["results"], imgIds=nb["imgIds"])
    stats = summarize_stats(ev, Params())
    assert capsys.readouterr().out.splitlines() == nb["printed"]
    assert np.array_equal(stats, ev["stats"])


def test_load_res_ids_area_and_image_subset(golden_dir):
    nb = _notebook(golden_dir)
    gt = COCO(nb["gt"])
    assert gt.getImgIds() == [558840] and gt.getCatIds() == list(range(80))
    dt = gt.loadRes(nb["results"])
    anns = dt.dataset["annotations"]
    assert [a["id"] for a in anns] == [1, 2, 3]
    assert [a["area"] for a in anns] == [r["bbox"][2] * r["bbox"][3] for r in nb["results"]]
    assert all(a["iscrowd"] == 0 for a in anns)
    assert dt.getImgIds() == [558840]
    bad = [dict(nb["results"][0], image_id=1)]
    with pytest.raises(AssertionError):
        gt.loadRes(bad)


def test_load_res_from_file(golden_dir, tmp_path):
    nb = _notebook(golden_dir)
    (tmp_path / "gt.json").write_text(json.dumps(nb["gt"]))
    (tmp_path / "res.json").write_text(json.dumps(nb["results"]))
    gt = COCO(str(tmp_path / "gt.json"))
    dt = gt.loadRes(str(tmp_path / "res.json"))
    assert len(dt.dataset["annotations"]) == 3 and dt.dataset["images"] == nb["gt"]["images"]


def test_unsupported_surface_raises(golden_dir):
    nb = _notebook(golden_dir)
    gt = COCO(nb["gt"])
    dt = gt.loadRes(nb["results"])
    with pytest.raises(NotImplementedError):
        COCOeval(gt, dt, 'segm')
    with pytest.raises(NotImplementedError):
        COCOeval(gt, dt, 'keypoints')
    e = COCOeval(gt, dt, 'bbox')
    assert e.params.imgIds == [558840] and e.params.catIds == list(range(80)) and e.params.useCats == 1
    assert np.array_equal(e.params.iouThrs, np.linspace(.5, .95, 10)) and np.array_equal(e.params.recThrs, np.linspace(0, 1, 101))
    assert e.params.maxDets == [1, 10, 100] and e.params.areaRng[0] == [0, 1e10]
    with pytest.raises(NotImplementedError):
        e.evalImgs
    e.params.useCats = 0
    with pytest.raises(NotImplementedError):
        e.evaluate()


def test_cocoeval_abi_layout_matches_the_c_header(tmp_path):
    """struct yv3_cocoeval_desc as ctypes sees it == as a C compiler sees include/yv3.h; the entry points are exported."""
    fields = [f for f, _ in _ffi.CocoEvalDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv3.h"\nint main(void){printf("%zu", sizeof(yv3_cocoeval_desc));\n'
                   + "".join('printf(" %%zu", offsetof(yv3_cocoeval_desc, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_ffi.CocoEvalDesc)] + [getattr(_ffi.CocoEvalDesc, f).offset for f in fields]
    lib = _ffi.lib()
    assert lib.yv3_cocoeval_workspace_bytes(10, 100, 5, 80, 4) > 0
    assert lib.yv3_cocoeval_workspace_bytes(10, 100, 0, 80, 4) == 0
    assert b"limit" in lib.yv3_error_string(_ffi.ELIMIT)


def test_cocoeval_rejects_limits_before_launching():
    """Argument limits are refused on the host side of the C entry point (no device work is enqueued)."""
    lib = _ffi.lib()
    d = _ffi.CocoEvalDesc()
    d.n_gt, d.n_det, d.n_img, d.n_cat = 0, 0, 1, 1
    d.n_iou, d.n_rec, d.n_area, d.n_maxdet = 10, 101, 7, 3          # 70 (t, a) lanes > 64
    d.max_dets[0], d.max_dets[1], d.max_dets[2] = 1, 10, 100
    assert lib.yv3_cocoeval(d, None, 0, None) == _ffi.ELIMIT
    d.n_area = 4
    d.max_dets[2] = 2000                                             # maxDets[-1] > 1024
    assert lib.yv3_cocoeval(d, None, 0, None) == _ffi.ELIMIT
    d.max_dets[2] = 5                                                # not ascending
    assert lib.yv3_cocoeval(d, None, 0, None) == -1                  # YV3_EINVAL


@pytest.mark.skipif(not __import__("importlib").util.find_spec("pycocotools"), reason="pycocotools not installed")
def test_restatement_matches_pycocotools(golden_dir):
    from pycocotools.coco import COCO as PCOCO
    from pycocotools.cocoeval import COCOeval as PCOCOeval
    import contextlib
    import io
    nb = _notebook(golden_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        gt = PCOCO()
        gt.dataset = nb["gt"]
        gt.createIndex()
        e = PCOCOeval(gt, gt.loadRes(nb["results"]), 'bbox')
        e.params.imgIds = nb["imgIds"]
        e.evaluate()
        e.accumulate()
        e.summarize()
    ev = cocoeval_np.evaluate(nb["gt"], nb["results"], imgIds=nb["imgIds"])
    for k in ("precision", "recall", "scores"):
        assert np.array_equal(ev[k], e.eval[k])
    assert np.array_equal(ev["stats"], e.stats)
