"""Golden fixture for the training augmentation (yolo_v3_amd/augment.py): what the REFERENCE's own transforms.py / boundingbox.py /
utils.py compute for the parts of the training transform that run without imgaug or cv2.

Build-container only (needs the reference checkout, given as the first argument).  cv2 and imgaug are absent: both are replaced by
stand-in modules whose classes accept any arguments and record them, so that ``iaa_hsv_aug`` runs for real and the values it hands
to ``iaa.Add`` / ``iaa.Multiply`` are read back.  Recorded:
  hsv_*        for a table of seeds: np.random.seed(seed) (dataset.py:181-186), then iaa_hsv_aug(hue, sat, exp)'s dhue, dsat, dexp
               (transforms.py:77-104), for two settings (darknet's 0.1 / 1.5 / 1.5 and a wider one)
  conv_*       BoundingBoxConverter.convert on a label table: relative cxcywh -> absolute x1y1x2y2 on (W, H), and back
  clip_*       bbs_clip / bbs_remove_cut_out(., 0.1) on a box table with a small stand-in box object: keep decisions, clipped boxes
  fill_*       ToTensor's label padding (fill_label_np_tensor, max_labels=90) of 0, 3, 90 and 130 rows

    python tools/make_golden_augment.py /path/to/reference      # rewrites tests/golden/augment.npz
"""
import os
import sys
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

RECORD = []


class _Rec:
    """Any stand-in class: records its constructor arguments."""

    def __init__(self, *args, **kwargs):
        self.args, self.kwargs = args, kwargs
        RECORD.append((type(self).__name__, args, kwargs))


class _StubModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (_Rec,), {})
        setattr(self, name, cls)
        return cls


class Box:
    """Stand-in for imgaug's BoundingBox: what bbs_clip reads (x1, y1, x2, y2, area, label) and copy()."""

    def __init__(self, x1, y1, x2, y2, label=None):
        self.x1, self.y1, self.x2, self.y2, self.label = x1, y1, x2, y2, label

    @property
    def area(self):
        return (self.y2 - self.y1) * (self.x2 - self.x1)

    def copy(self, x1, y1, x2, y2, label):
        return Box(x1, y1, x2, y2, label)


class Boxes:
    def __init__(self, bounding_boxes, shape):
        self.bounding_boxes, self.shape = bounding_boxes, shape


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    for n in ["cv2", "imgaug", "imgaug.augmenters", "torchvision", "torchvision.transforms", "torchvision.datasets",
              "torchvision.models"]:
        sys.modules[n] = _StubModule(n)
    sys.modules["imgaug"].augmenters = sys.modules["imgaug.augmenters"]
    sys.modules["imgaug"].BoundingBoxesOnImage = Boxes
    tv = sys.modules["torchvision"]
    tv.transforms, tv.datasets, tv.models = (sys.modules["torchvision." + k] for k in ("transforms", "datasets", "models"))
    warnings.simplefilter("ignore")
    import transforms as ref                                             # the reference's transforms.py
    from boundingbox import BoundingBoxConverter, CoordinateType, FormatType

    out = {}
    # -- colour draws, in iaa_hsv_aug's own order
    seeds = np.array([0, 1, 2, 3, 7, 42, 123, 999, 2 ** 20 + 5, 2 ** 31 - 2, 31337, 65535], dtype=np.int64)
    for tag, (hue, sat, exp) in (("darknet", (0.1, 1.5, 1.5)), ("wide", (0.3, 2.0, 3.0))):
        vals = []
        for s in seeds:
            np.random.seed(int(s))
            del RECORD[:]
            ref.iaa_hsv_aug(hue, sat, exp)
            add = [r for r in RECORD if r[0] == "Add"]
            mul = [r for r in RECORD if r[0] == "Multiply"]
            dhue = add[0][1][0][0]
            dsat, dexp = mul[0][1][0][0], mul[1][1][0][0]
            assert add[0][1][0][0] == add[0][1][0][1] and mul[0][1][0][0] == mul[0][1][0][1]
            vals.append((dhue, dsat, dexp))
        out["hsv_" + tag] = np.array(vals, dtype=np.float64)
        out["hsv_" + tag + "_settings"] = np.array((hue, sat, exp), dtype=np.float64)
    out["hsv_seeds"] = seeds

    # -- BoundingBoxConverter.convert both ways (IaaAugmentations.__call__, transforms.py:52-73)
    rng = np.random.RandomState(5)
    lab = np.zeros((24, 5), dtype=np.float64)
    lab[:, 0] = rng.randint(0, 80, 24)
    lab[:, 1:3] = rng.uniform(0.0, 1.0, (24, 2))
    lab[:, 3:5] = rng.uniform(0.0, 0.9, (24, 2))
    lab[3, 3] = 0.0                                                      # degenerate rows (dropped by label_np_to_bbs)
    lab[5, 4] = 0.0
    lab[7] = 0.0                                                         # a zero padding row
    dims = np.array([(640, 480), (333, 500), (1, 1), (97, 1231)], dtype=np.int64)     # (W, H)
    fwd, back = [], []
    for (W, H) in dims:
        a = BoundingBoxConverter.convert(lab, CoordinateType.Relative, FormatType.cxcywh, CoordinateType.Absolute,
                                         FormatType.x1y1x2y2, bbox_idx=[1, 2, 3, 4], img_dim=(int(W), int(H)))
        fwd.append(a)
        back.append(BoundingBoxConverter.convert(a, CoordinateType.Absolute, FormatType.x1y1x2y2, CoordinateType.Relative,
                                                 FormatType.cxcywh, bbox_idx=[1, 2, 3, 4], img_dim=(int(W), int(H))))
    out["conv_labels"], out["conv_dims"] = lab, dims
    out["conv_abs"], out["conv_back"] = np.array(fwd), np.array(back)

    # -- bbs_clip / bbs_remove_cut_out(., 0.1) on canvas shapes
    boxes = [(10, 10, 50, 60), (-30, 5, 20, 40), (-100, -100, 5, 5), (400, 400, 430, 420), (410, 0, 500, 416),
             (0, 0, 416, 416), (-1, -1, 417, 417), (380, 100, 420, 150), (380.5, 100.25, 420.75, 150.5), (-4.5, 3, 0.5, 9),
             (415.9, 200, 416.1, 210), (100, -45, 140, 5), (100, -44.9, 140, 5.1), (0.0, 0.0, 1e-3, 1e-3), (-10, 200, 1, 300)]
    shapes = np.array([(416, 416), (608, 608), (416, 608)], dtype=np.int64)  # (height, width)
    keep, clipped = [], []
    for (h, w) in shapes:
        bbs = Boxes([Box(*b, label=np.array([float(i), 0, 0, 0, 0])) for i, b in enumerate(boxes)], (int(h), int(w), 3))
        res = ref.bbs_remove_cut_out(bbs, 0.1)
        kept = {int(b.label[0]): b for b in res.bounding_boxes}
        keep.append([i in kept for i in range(len(boxes))])
        clipped.append([(float(kept[i].x1), float(kept[i].y1), float(kept[i].x2), float(kept[i].y2)) if i in kept
                        else (np.nan,) * 4 for i in range(len(boxes))])
    out["clip_boxes"], out["clip_shapes"] = np.array(boxes, dtype=np.float64), shapes
    out["clip_keep"], out["clip_out"] = np.array(keep), np.array(clipped, dtype=np.float64)

    # -- ToTensor's label padding
    for n in (0, 3, 90, 130):
        rows = np.arange(n * 5, dtype=np.float64).reshape(n, 5) + 1.0
        t = ref.ToTensor()({"img": None, "label": rows if n else np.array([])})["label"]
        out["fill_%d_in" % n], out["fill_%d_out" % n] = rows, t.numpy()

    np.savez_compressed(os.path.join(GOLD, "augment.npz"), **out)
    print("wrote augment.npz:", ", ".join("%s%s" % (k, tuple(v.shape)) for k, v in out.items()))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_augment.py REFERENCE_DIR")
    main(sys.argv[1])
