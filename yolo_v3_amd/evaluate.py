"""COCO ground-truth and results writers of the reference's ``evaluate.py``, the results fed by the GPU hot path.

Ground truth (reference evaluate.py:38-115, ``generate_annotations_file`` and its helpers): same names, arguments, entry
layout and bytes on disk (``json.dump(d, f, indent=4, separators=(',', ':'))``); darknet label files (``cls cx cy w h``,
relative) become absolute ``xywh`` with the reference's float64 operation order (boundingbox.py:30-33,45-48,59-80),
``area = w*h``, ``iscrowd = 0``, annotation ids ``0, 1, 2, ...`` (the first id is 0: see ``yolo_v3_amd.cocoeval`` on what
that does to the score).  One difference: an image without a label file has no annotations (the reference reuses the
previous image's labels, or raises ``NameError`` on the first image).  Image sizes are those of the decoded, EXIF-rotated
image, as ``cv2.imread`` and `read_image_rgb` see it.

Results:

Mirrors reference evaluate.py:117-121 (``create_results_entry``), :151-195 (``open_json_pred_writer``,
``JsonPredictionWriter``) and :197-206 (``predict_and_process``): same names, arguments, entry layout
(``image_id, category_id, bbox [x,y,w,h] in ORIGINAL-image pixels, score``), same on-disk byte format
(``json.dump(entry, indent=4, separators=(',', ':'))`` joined by ``,`` inside ``[...]``).  Differences:

* the boxes of a whole batch are un-letterboxed / rescaled by ONE ``yv3_correct_boxes`` launch
  (``csrc/prepost.hip``) instead of one torch expression per image;
* ``predict_and_process`` runs the fused GPU ``detect`` (eval mode: conf 0.005, nms 0.45, evaluate.py:201-204);
* a run without a single detection writes ``[]`` (the reference's seek-back-one-byte leaves ``]``, invalid JSON).

``image_id`` comes from the trailing digits of the file name (reference utils.py:294-297); ``category_id`` is the
class index 0..C-1 as in the reference (it never maps to COCO's sparse ids).
"""
import json
import os.path as osp
import re
import warnings
from collections import OrderedDict
from contextlib import contextmanager

import numpy as np
import torch

from . import _ffi


def get_image_id_from_path(image_path):
    """reference utils.py:294-297"""
    image_path = osp.splitext(image_path)[0]
    m = re.search(r'\d+$', image_path)
    return int(m.group())


def create_annotations(cat_list, img_list, ann_list):
    """reference evaluate.py:42-45"""
    return OrderedDict({'categories': cat_list, 'images': img_list, 'annotations': ann_list})


def create_images_entry(image_id, width=None, height=None):
    """reference evaluate.py:47-51"""
    if width is None or height is None:
        return OrderedDict({'id': image_id})
    return OrderedDict({'id': image_id, 'width': width, 'height': height})


def create_categories(class_names):
    """reference evaluate.py:53-54"""
    return [{'id': i, 'name': cls} for i, cls in enumerate(class_names)]


def create_annotations_entry(image_id, bbox, category_id, ann_id, iscrowd=0, area=None, segmentation=None):
    """reference evaluate.py:56-71"""
    if area is None:
        if segmentation is None:
            area = bbox[2] * bbox[3]
        else:
            raise NotImplementedError()
    return OrderedDict({"id": ann_id, "image_id": image_id, "category_id": category_id, "iscrowd": iscrowd, "area": area,
                        "bbox": bbox})


def generate_annotations_file(target_txt, class_names, out):
    """reference evaluate.py:73-76: the COCO ground-truth file of the images listed in ``target_txt``."""
    ann_dict = create_annotations_dict(target_txt, class_names)
    with open(out, 'w') as f:
        json.dump(ann_dict, f, indent=4, separators=(',', ':'))


def create_annotations_dict(target_txt, class_names):
    """reference evaluate.py:78-87: label path = image path with every ``jpg`` -> ``txt`` and every ``images`` -> ``labels``."""
    with open(target_txt, 'r') as f:
        img_path_list = [lines.strip() for lines in f.readlines()]
    label_path_list = [img_path.replace('jpg', 'txt').replace('images', 'labels') for img_path in img_path_list]
    img_list, ann_list = get_img_ann_list(img_path_list, label_path_list)
    cat_list = create_categories(class_names)
    return create_annotations(cat_list, img_list, ann_list)


def image_size(path):
    """(width, height) of the decoded image after its EXIF orientation is applied -- the shape `read_image_rgb` returns and
    ``cv2.imread`` gives, read from the header without decoding the pixels (orientations 5-8 swap the axes)."""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
        orientation = im.getexif().get(0x0112, 1)
    return (h, w) if orientation in (5, 6, 7, 8) else (w, h)


def labels_to_xywh(labels, width, height):
    """Darknet rows ``cls cx cy w h`` (relative) -> ``cls x y w h`` (absolute), float64, in the reference's order:
    BoundingBoxConverter.convert (boundingbox.py:59-80) = cxcywh -> xywh (x = cx - w/2, y = cy - h/2) on the relative
    values, then x, w *= width and y, h *= height."""
    labels = np.array(labels, dtype=np.float64).reshape(-1, 5)
    if len(labels) == 0:
        return labels
    box = labels[..., [1, 2, 3, 4]]
    x, y = box[..., 0] - box[..., 2] / 2, box[..., 1] - box[..., 3] / 2
    box[..., 0], box[..., 1] = x, y
    box[..., [0, 2]] *= width
    box[..., [1, 3]] *= height
    labels[..., 1:5] = box
    return labels


def get_img_ann_list(img_path_list, label_path_list):
    """reference evaluate.py:89-115: one images entry per path, one annotation per label row, ids in order from 0.
    A missing label file means "no annotations" (the one difference from the reference, see the module docstring)."""
    img_list, ann_list = [], []
    for img_path, label_path in zip(img_path_list, label_path_list):
        image_id = get_image_id_from_path(img_path)
        width, height = image_size(img_path)
        img_list.append(create_images_entry(image_id, width, height))
        if not osp.exists(label_path):
            continue
        with warnings.catch_warnings():                    # (an empty label file: "input contained no data")
            warnings.simplefilter("ignore", UserWarning)
            rows = np.loadtxt(label_path).reshape(-1, 5)
        labels = labels_to_xywh(rows, width, height)
        for label in labels:
            category_id = int(label[0])
            bbox = list(label[1:5])
            ann_id = len(ann_list)
            ann_list.append(create_annotations_entry(image_id, bbox, category_id, ann_id))
    return img_list, ann_list


def create_results_entry(image_id, category_id, bbox, score):
    """reference evaluate.py:117-121"""
    return OrderedDict({"image_id": image_id, "category_id": category_id, "bbox": bbox, "score": score})


class BatchHandler:
    def process_batch(self, sample, predictions):
        raise NotImplementedError


def _wh(img):
    # CHW tensors as the reference's ToTensor produces (evaluate.py:182); HWC uint8 arrays also accepted
    s = tuple(img.shape)
    return (s[2], s[1]) if (len(s) == 3 and s[0] in (1, 3) and s[2] not in (1, 3)) else (s[1], s[0])


def correct_batch(sample, predictions, is_letterbox):
    """The boxes of a batch mapped back to the ORIGINAL images by one ``yv3_correct_boxes`` launch: ``(host, counts, xywh)`` --
    the predictions padded to CPU ``[B, cap, 7]``, the per-image counts and the corrected CPU ``[B, cap, 4]`` boxes ``x, y, w, h``
    -- or None when no image of the batch has a detection."""
    imgs, org_imgs, img_paths = sample['img'], sample['org_img'], sample['img_path']
    B = len(img_paths)
    preds = [predictions[i] if (i < len(predictions) and predictions[i] is not None) else torch.Tensor() for i in range(B)]
    counts = [int(p.shape[0]) if p.numel() else 0 for p in preds]
    cap = max(counts) if counts else 0
    if cap == 0:
        return None
    if not torch.cuda.is_available():
        raise _ffi.Yv3Error("no GPU available: this package has no CPU path")
    img_w, img_h = _wh(imgs[0])
    # one launch for the whole batch: padded [B, cap, 7] boxes + per-image counts + original sizes
    host = torch.zeros((B, cap, 7), dtype=torch.float32)
    for i, p in enumerate(preds):
        if counts[i]:
            host[i, :counts[i]] = p.detach().float().cpu()[:, :7]
    org = torch.tensor([list(_wh(o)) for o in org_imgs], dtype=torch.int32)
    dev = torch.device("cuda")
    boxes, cnt, orgd = host.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), org.to(dev)
    out = torch.empty((B, cap, 4), dtype=torch.float32, device=dev)
    _ffi.check(_ffi.lib().yv3_correct_boxes(boxes.data_ptr(), B, cap, 7, cnt.data_ptr(), orgd.data_ptr(), int(img_w), int(img_h),
                                            int(bool(is_letterbox)), 0, out.data_ptr(), _ffi.stream_ptr()),
               "yv3_correct_boxes")
    return host, counts, out.cpu()


class JsonPredictionWriter(BatchHandler):
    """reference evaluate.py:164-195"""

    def __init__(self, out_path, classes_names, is_letterbox=False):
        self.out_path = out_path
        self.file = open(out_path, 'w')
        self.classes_names = classes_names
        self.is_letterbox = is_letterbox
        self.entries = 0

    def write_start(self):
        self.file.write('[')

    def write_end(self):
        self.file.write(']')
        self.file.close()

    _wh = staticmethod(_wh)

    def process_batch(self, sample, predictions):
        img_paths = sample['img_path']
        corrected = correct_batch(sample, predictions, self.is_letterbox)
        if corrected is None:
            return
        host, counts, xywh = corrected
        for i in range(len(img_paths)):
            image_id = get_image_id_from_path(img_paths[i])
            for j in range(counts[i]):
                res = create_results_entry(image_id, int(host[i, j, 6].item()), xywh[i, j].tolist(), host[i, j, 5].item())
                if self.entries:
                    self.file.write(',')
                json.dump(res, self.file, indent=4, separators=(',', ':'))
                self.entries += 1


@contextmanager
def open_json_pred_writer(out_path, classes_names, is_letterbox=False):
    """reference evaluate.py:151-158"""
    pred_writer = JsonPredictionWriter(out_path, classes_names, is_letterbox)
    try:
        pred_writer.write_start()
        yield pred_writer
    finally:
        pred_writer.write_end()


def predict_and_process(data, net, num_classes, batch_handler=None, obj_conf_thr=0.005, nms_thr=0.45):
    """reference evaluate.py:197-206: eval-mode detection (is_eval=True; the reference's fixed thresholds conf 0.005 /
    nms 0.45 are the defaults) over an iterable of samples ``{'img': [B,3,H,W] tensor, 'org_img': [...],
    'img_path': [...]}``, each batch handed to ``batch_handler``.  The GPU NMS handles up to ~5e5 (row, class)
    candidates per image and fails loudly beyond (untrained / synthetic weights at conf 0.005 can exceed that)."""
    from .detect import detect
    with torch.no_grad():
        for sample in data:
            predictions = detect(net, sample['img'].cuda(), num_classes, obj_conf_thr=obj_conf_thr, nms_thr=nms_thr,
                                 is_eval=True, use_nms=True)
            if predictions == []:
                predictions = [torch.Tensor() for _ in sample['img_path']]
            batch_handler.process_batch(sample, predictions)


def read_image_rgb(path):
    """uint8 RGB [H,W,3] of an image file (the reference reads with ``cv2.imread`` + BGR->RGB, evaluate.py:136-137; cv2 is not a
    dependency here: PIL decodes -- JPEG decoders may differ from OpenCV's by an LSB on some pixels).  ``cv2.imread`` applies the
    file's EXIF orientation by default (IMREAD_COLOR without IMREAD_IGNORE_ORIENTATION); PIL does not, so it is applied here
    (``ImageOps.exif_transpose``): COCO holds JPEGs with an orientation tag, and both the pixels fed to the network and the
    org_w / org_h the boxes are mapped back with must be the rotated image's, as in the reference."""
    import numpy as np
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        im = ImageOps.exif_transpose(im)
        return np.asarray(im.convert("RGB"), dtype=np.uint8).copy()


def image_batches(target_txt, bs, dim, is_letterbox=False, decode="pil", entropy="serial", progressive=False):
    """The samples `generate_results_file` and `annotate_images` feed to the network, ``bs`` images at a time:
    ``{'img': [B,3,h,w] GPU tensor, 'org_img': the original images (HWC uint8: arrays, or GPU tensors with decode="gpu"),
    'img_path': [...]}``.  ``target_txt``: the reference's text file with one image path per line, or a list of paths or of
    ``(path, uint8 RGB [H,W,3] array)`` pairs."""
    from .utils import letterbox_batch
    if isinstance(target_txt, str):
        with open(target_txt, 'r') as f:
            items = [line.strip() for line in f.readlines() if line.strip()]
    else:
        items = list(target_txt)

    def batches():                                                  # (the list is read before the first batch is asked for)
        for i in range(0, len(items), bs):
            chunk = items[i:i + bs]
            paths = [c if isinstance(c, str) else c[0] for c in chunk]
            if decode == "gpu":
                from . import jpeg
                files = iter(jpeg.decode_batch([c for c in chunk if isinstance(c, str)], entropy=entropy, progressive=progressive))
                imgs = [next(files) if isinstance(c, str) else c[1] for c in chunk]
            else:
                imgs = [read_image_rgb(c) if isinstance(c, str) else c[1] for c in chunk]
            x, _ = letterbox_batch(imgs, dim, variant="eval" if is_letterbox else "scale")
            yield {"img": x, "org_img": imgs, "img_path": paths}    # (the writers need the ORIGINAL images: HWC)

    return batches()


def generate_results_file(net, target_txt, classes_names, out, bs, dim, is_letterbox=False, decode="pil", entropy="serial",
                          progressive=False):
    """reference evaluate.py:208-219: the COCO-results file of a list of images -- ``target_txt`` is the reference's text file with one
    image path per line (a list of paths, or of ``(path, uint8 RGB [H,W,3] array)`` pairs, is accepted too).  Per batch of ``bs``
    images: the evaluation pipeline's input preparation on the GPU (``IaaLetterbox(dim)`` when ``is_letterbox`` else
    ``iaa.Scale(dim)``, then ``ToTensor``: `utils.letterbox_batch(variant="eval" | "scale")`), eval-mode detection (conf 0.005 / nms
    0.45) and the writer.  ``dim`` = (w, h).  Returns the number of result entries written.

    ``decode="gpu"``: each batch's files are decoded by `jpeg.decode_batch` instead of `read_image_rgb` in this thread -- the same
    pixels (files the GPU decoder does not take still go through `read_image_rgb`), so the same file.  ``entropy`` is passed on to
    it (``"serial"`` or ``"parallel"``; it changes no pixel), and so is ``progressive`` (True: accepted progressive files are
    decoded on the GPU too)."""
    if decode not in ("pil", "gpu"):
        raise ValueError("decode must be 'pil' or 'gpu'")
    if entropy not in ("serial", "parallel"):
        raise ValueError("entropy must be 'serial' or 'parallel'")
    numclass = len(classes_names)
    batches = image_batches(target_txt, bs, dim, is_letterbox, decode, entropy, progressive)

    with open_json_pred_writer(out, classes_names, is_letterbox) as pred_writer:
        predict_and_process(batches, net, num_classes=numclass, batch_handler=pred_writer)
        return pred_writer.entries


class JpegAnnotationWriter(BatchHandler):
    """Annotated frames out (what the reference shows with ``test.py:predict`` / ``show_detections`` and ``draw.py``): per batch the
    boxes are corrected as `JsonPredictionWriter` corrects them, drawn on the ORIGINAL-size images with their class names
    (`draw.draw_boxes`: box j in colour ``palette[class]``, outline then label tag, in detection order) and the images are encoded
    on the GPU (`jpeg.encode_batch`) and written to ``out_dir/<image stem>.jpg``.  Only the box integers go to the device and only
    the compressed bytes come back; original images that are GPU tensors (``decode="gpu"``) never leave it, host arrays are
    uploaded.  An image without detections is written without boxes.  ``written``: the paths written so far; ``boxes``: per
    written file its ``(rectangles, classes)``, int32 ``[n, 4]`` / int ``[n]``, as drawn."""

    def __init__(self, out_dir, classes_names, is_letterbox=False, quality=75, subsampling="4:2:0", thickness=2):
        from . import draw
        self.out_dir, self.classes_names, self.is_letterbox = out_dir, list(classes_names), is_letterbox
        self.quality, self.subsampling, self.thickness = quality, subsampling, thickness
        self.atlas = draw.LabelAtlas(self.classes_names)
        self.palette = draw.palette(len(self.classes_names))
        self.written, self.boxes = [], []

    def process_batch(self, sample, predictions):
        from . import draw, jpeg
        org_imgs, img_paths = sample['org_img'], sample['img_path']
        B = len(img_paths)
        if not torch.cuda.is_available():
            raise _ffi.Yv3Error("no GPU available: this package has no CPU path")
        corrected = correct_batch(sample, predictions, self.is_letterbox)
        rects, classes = [np.zeros((0, 4), np.int32)] * B, [np.zeros(0, np.int64)] * B
        if corrected is not None:
            host, counts, xywh = corrected
            rects = [draw.rectangles(xywh[i, :counts[i]].numpy()) for i in range(B)]
            classes = [host[i, :counts[i], 6].numpy().astype(np.int64) for i in range(B)]
        # the drawing is in place: on a copy, so that the caller's originals (the decoder's buffer, with decode="gpu") stay as they were
        frames = [o.clone() if isinstance(o, torch.Tensor) and o.is_cuda else torch.as_tensor(np.ascontiguousarray(o)).cuda() for o in org_imgs]
        draw.draw_boxes(frames, rects, [self.palette[c] for c in classes], classes, self.atlas, thickness=self.thickness)
        files = jpeg.encode_batch(frames, quality=self.quality, subsampling=self.subsampling)
        for path, data, r, c in zip(img_paths, files, rects, classes):
            out = osp.join(self.out_dir, osp.splitext(osp.basename(path))[0] + ".jpg")
            with open(out, "wb") as f:
                f.write(data)
            self.written.append(out)
            self.boxes.append((r, c))


def annotate_images(net, target_txt, classes_names, out_dir, bs, dim, is_letterbox=False, decode="pil", obj_conf_thr=0.5, nms_thr=0.4,
                    quality=75):
    """Detect, draw and encode the images listed in ``target_txt`` (as `generate_results_file` takes it), ``bs`` at a time, and
    write ``out_dir/<image stem>.jpg`` for each: the original image with its boxes and class names on it.  ``dim`` = (w, h) of the
    network input; ``obj_conf_thr`` / ``nms_thr`` are the detection thresholds.  ``decode="gpu"``: the files are decoded by
    `jpeg.decode_batch` and the originals stay on the device from decode to encode (files that decoder hands to PIL are uploaded).
    Returns the `JpegAnnotationWriter`, whose ``written`` lists the files."""
    if decode not in ("pil", "gpu"):
        raise ValueError("decode must be 'pil' or 'gpu'")
    import os
    os.makedirs(out_dir, exist_ok=True)
    writer = JpegAnnotationWriter(out_dir, classes_names, is_letterbox, quality=quality)
    predict_and_process(image_batches(target_txt, bs, dim, is_letterbox, decode), net, num_classes=len(classes_names), batch_handler=writer,
                        obj_conf_thr=obj_conf_thr, nms_thr=nms_thr)
    return writer
