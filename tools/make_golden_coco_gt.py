"""Golden fixtures for COCO bbox evaluation, made from the reference (build container only: needs the reference checkout).

1. The ground-truth writer: runs the REFERENCE's ``evaluate.generate_annotations_file`` (evaluate.py:73-115) on six synthetic
   images with darknet label files -- several classes, an empty label file, boxes touching the border.  ``evaluate.cv2.imread``
   is patched to return arrays of the chosen shapes; the reference's stand-in-module import is the one of
   ``oracle/make_golden_coco.py`` (imported, not changed).  Writes ``tests/golden/coco_gt_ref.json`` (the reference's bytes)
   and ``tests/golden/coco_gt_inputs.json`` (file names, image sizes, label texts).
2. The notebook's toy case (``evaluate.ipynb`` cells 9-25): the ground truth and results the notebook builds, run through the
   notebook's own cell sources, and the 12 lines cell 25 printed.  Writes ``tests/golden/cocoeval_notebook.json``.

    python tools/make_golden_coco_gt.py [REFERENCE_DIR]
"""
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLD = os.path.join(REPO, "tests", "golden")

# (file name, (width, height), label text)
IMAGES = [
    ("COCO_val2014_000000000139.jpg", (640, 427),
     "0 0.5 0.5 0.25 0.4\n56 0.1 0.2 0.2 0.4\n56 0.333 0.667 0.125 0.0625\n"),
    ("COCO_val2014_000000000285.jpg", (586, 640), ""),                                        # empty label file
    ("COCO_val2014_000000000632.jpg", (640, 483),
     "62 0.5 0.5 1.0 1.0\n3 0.05 0.95 0.1 0.1\n79 0.999 0.001 0.002 0.002\n"),               # border-touching boxes
    ("COCO_val2014_000000000724.jpg", (375, 500), "11 0.41733333 0.52 0.30133333 0.617\n"),
    ("COCO_val2014_000000000776.jpg", (428, 640),
     "0 0.2 0.3 0.1 0.1\n0 0.21 0.31 0.1 0.1\n44 0.75 0.25 0.5 0.5\n27 0.6 0.6 0.05 0.3\n"),
    ("COCO_val2014_000000001000.jpg", (1920, 1080), "17 0.123456789 0.987654321 0.0123 0.0246\n"),
]


def reference_evaluate(ref):
    from oracle import make_golden_coco as mgc                  # its stand-in modules for cv2 / imgaug / torchvision / ...
    sys.path.insert(0, ref)
    for n in ["cv2", "imgaug", "imgaug.augmenters", "torchvision", "torchvision.transforms", "torchvision.datasets",
              "torchvision.models", "draw", "transforms", "dataset"]:
        sys.modules[n] = mgc._Anything(n)
    sys.modules["imgaug"].augmenters = sys.modules["imgaug.augmenters"]
    tv = sys.modules["torchvision"]
    tv.transforms, tv.datasets, tv.models = (sys.modules["torchvision." + k] for k in ("transforms", "datasets", "models"))
    import warnings
    warnings.simplefilter("ignore")
    import evaluate
    return evaluate


def make_gt(evaluate, names):
    sizes = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "coco")
        os.makedirs(os.path.join(root, "images"))
        os.makedirs(os.path.join(root, "labels"))
        paths = []
        for name, (w, h), text in IMAGES:
            p = os.path.join(root, "images", name)
            open(p, "wb").close()
            with open(p.replace("jpg", "txt").replace("images", "labels"), "w") as f:
                f.write(text)
            sizes[p] = (h, w)
            paths.append(p)
        target = os.path.join(tmp, "list.txt")
        with open(target, "w") as f:
            f.write("\n".join(paths) + "\n")
        evaluate.cv2.imread = lambda p: np.zeros(sizes[p] + (3,), dtype=np.uint8)
        out = os.path.join(GOLD, "coco_gt_ref.json")
        evaluate.generate_annotations_file(target, names, out)
    with open(os.path.join(GOLD, "coco_gt_inputs.json"), "w") as f:
        json.dump({"class_names": names, "images": [{"file": n, "width": w, "height": h, "labels": t} for n, (w, h), t in IMAGES]},
                  f, indent=1)
    print("wrote", out, os.path.getsize(out), "bytes")


def make_notebook(ref, names):
    nb = json.load(open(os.path.join(ref, "evaluate.ipynb")))
    cells = nb["cells"]
    src = lambda i: "".join(cells[i]["source"])
    env = {"OrderedDict": __import__("collections").OrderedDict, "classes": names}
    for i in (9, 10, 11, 12, 13, 14, 17, 18, 19):               # GT entries, categories, results entries
        exec(src(i), env)
    printed = [ln for ln in "".join(cells[25]["outputs"][0]["text"]).splitlines() if ln.startswith(" Average")]
    assert len(printed) == 12, printed
    imgIds = sorted(set(r["image_id"] for r in env["coco_results"]))     # cell 24: sorted(cocoDt.getImgIds())
    out = {"source": "evaluate.ipynb cells 9-25", "gt": env["anno_json"], "results": env["coco_results"], "imgIds": imgIds,
           "printed": printed, "stats": [float(ln.rsplit("=", 1)[1]) for ln in printed]}
    p = os.path.join(GOLD, "cocoeval_notebook.json")
    with open(p, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", p)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    with open(os.path.join(ref, "data", "coco.names")) as f:
        names = [line.rstrip("\n") for line in f.readlines()]
    names = [n for n in names if n]
    make_notebook(ref, names)
    make_gt(reference_evaluate(ref), names[:80])


if __name__ == "__main__":
    main()
