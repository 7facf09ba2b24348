"""COCO bbox mAP on the GPU: the subset of pycocotools (2.0.x) the reference notebook uses (evaluate.ipynb cells 22-25, 48-56).

    from yolo_v3_amd.cocoeval import COCO, COCOeval      # instead of pycocotools.coco / pycocotools.cocoeval
    cocoGt = COCO("coco_valid.json")                     # evaluate.generate_annotations_file
    cocoDt = cocoGt.loadRes("coco_valid_result.json")    # evaluate.generate_results_file
    cocoEval = COCOeval(cocoGt, cocoDt, 'bbox')
    cocoEval.params.imgIds = sorted(cocoDt.getImgIds())
    cocoEval.evaluate(); cocoEval.accumulate(); cocoEval.summarize()
    cocoEval.stats                                       # the 12 AP / AR numbers

The host parses JSON and maps image / category ids to dense indices; grouping, matching, ordering and accumulation run in
``yv3_cocoeval`` (csrc/cocoeval.hip), bit-identical to pycocotools' float64 arithmetic.  ``summarize`` runs on the host.

Kept from pycocotools on purpose: a detection matched to a ground-truth annotation whose id is 0 counts as unmatched (a false
positive unless ignored) while that annotation is still used up.  ``evaluate.generate_annotations_file`` numbers annotations
from 0, as the reference does, so the first annotation of such a file never counts as found.

Not implemented (``NotImplementedError``): ``iouType`` other than ``'bbox'``, ``params.useCats = 0``, the per-image
``evalImgs`` records, ``accumulate(p)`` with other parameters.

`evaluate_detections` scores ``detect()`` outputs against per-image boxes directly, without files.
"""
import copy
import json
import time

import numpy as np
import torch

from . import _ffi


class COCO:
    """pycocotools.coco.COCO, bbox subset: ``dataset``, ``getImgIds``, ``getCatIds``, ``loadRes``."""

    def __init__(self, annotation_file=None):
        self.dataset = {}
        if isinstance(annotation_file, dict):
            self.dataset = annotation_file
        elif annotation_file is not None:
            with open(annotation_file, 'r') as f:
                self.dataset = json.load(f)
            if not isinstance(self.dataset, dict):
                raise TypeError("annotation file format %s not supported" % type(self.dataset))
        self.createIndex()

    def createIndex(self):
        self.anns = {a['id']: a for a in self.dataset.get('annotations', [])}
        self.imgs = {im['id']: im for im in self.dataset.get('images', [])}
        self.cats = {c['id']: c for c in self.dataset.get('categories', [])}

    def getImgIds(self, imgIds=[], catIds=[]):
        ids = list(self.imgs.keys())
        if imgIds:
            ids = [i for i in ids if i in set(imgIds)]
        if catIds:
            keep = set(catIds)
            with_cat = set(a['image_id'] for a in self.dataset.get('annotations', []) if a['category_id'] in keep)
            ids = [i for i in ids if i in with_cat]
        return ids

    def getCatIds(self):
        return [c['id'] for c in self.dataset.get('categories', [])]

    def loadRes(self, resFile):
        """Results (a file name or a list of ``{image_id, category_id, bbox, score}``) as a COCO object: ``id`` = position + 1,
        ``area`` = w * h, ``iscrowd`` = 0.  Every result's image must be one of this object's images."""
        res = COCO()
        res.dataset['images'] = [img for img in self.dataset.get('images', [])]
        if isinstance(resFile, str):
            with open(resFile) as f:
                anns = json.load(f)
        else:
            anns = resFile
        if not isinstance(anns, list):
            raise TypeError("results must be a list of annotations")
        if not set(a['image_id'] for a in anns) <= set(self.getImgIds()):
            raise AssertionError("Results do not correspond to current coco set")
        res.dataset['categories'] = copy.deepcopy(self.dataset.get('categories', []))
        out = []
        for i, ann in enumerate(anns):
            if 'bbox' not in ann or ann['bbox'] == []:
                raise NotImplementedError("only bbox results are supported")
            bb = ann['bbox']
            ann = dict(ann)
            ann['area'] = bb[2] * bb[3]
            ann['id'] = i + 1
            ann['iscrowd'] = 0
            out.append(ann)
        res.dataset['annotations'] = out
        res.createIndex()
        return res


class Params:
    """pycocotools.cocoeval.Params, detection defaults."""

    def __init__(self, iouType='bbox'):
        if iouType != 'bbox':
            raise NotImplementedError("only iouType 'bbox' is supported")
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1
        self.iouType = iouType


def _dense(ids, keys):
    """Position of each id in the sorted unique ``keys``, -1 where absent."""
    ids = np.asarray(ids, dtype=np.int64)
    if keys.size == 0 or ids.size == 0:
        return np.full(ids.shape, -1, dtype=np.int32)
    pos = np.minimum(np.searchsorted(keys, ids), keys.size - 1)
    return np.where(keys[pos] == ids, pos, -1).astype(np.int32)


def _pack(arrays):
    """One contiguous host buffer (256-byte aligned members) -> (uint8 array, offsets)."""
    offs, o = [], 0
    for a in arrays:
        offs.append(o)
        o += (a.nbytes + 255) & ~255
    buf = np.zeros(max(o, 256), dtype=np.uint8)
    for a, off in zip(arrays, offs):
        buf[off:off + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return buf, offs


def run_device(gt_img, gt_cat, gt_box, gt_area, gt_crowd, gt_id, det_img, det_cat, det_box, det_score, n_img, n_cat,
               iouThrs, recThrs, areaRng, maxDets, timings=None):
    """``yv3_cocoeval`` on dense host arrays (see include/yv3.h); returns float64 ``precision`` [T,R,K,A,M], ``recall``
    [T,K,A,M], ``scores`` [T,R,K,A,M].  ``timings`` (a dict) receives the H2D / device / D2H times in seconds."""
    if not torch.cuda.is_available():
        raise _ffi.Yv3Error("no GPU available: this package has no CPU path")
    iouThrs = np.ascontiguousarray(iouThrs, dtype=np.float64)
    recThrs = np.ascontiguousarray(recThrs, dtype=np.float64)
    areaRng = np.ascontiguousarray(areaRng, dtype=np.float64).reshape(-1, 2)
    maxDets = [int(m) for m in maxDets]
    T, R, A, M, K = len(iouThrs), len(recThrs), len(areaRng), len(maxDets), int(n_cat)
    if M > _ffi.COCO_MAX_MAXDETS:
        raise _ffi.Yv3Error("yv3_cocoeval: at most %d maxDets values" % _ffi.COCO_MAX_MAXDETS)
    host = [np.ascontiguousarray(gt_img, np.int32), np.ascontiguousarray(gt_cat, np.int32),
            np.ascontiguousarray(gt_box, np.float64).reshape(-1, 4), np.ascontiguousarray(gt_area, np.float64),
            np.ascontiguousarray(gt_crowd, np.int32), np.ascontiguousarray(gt_id, np.int64),
            np.ascontiguousarray(det_img, np.int32), np.ascontiguousarray(det_cat, np.int32),
            np.ascontiguousarray(det_box, np.float64).reshape(-1, 4), np.ascontiguousarray(det_score, np.float64),
            iouThrs, recThrs, areaRng]
    n_gt, n_det = len(host[0]), len(host[6])
    buf, offs = _pack(host)
    lib = _ffi.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    ws_bytes = lib.yv3_cocoeval_workspace_bytes(n_gt, n_det, int(n_img), K, A)
    if ws_bytes == 0:
        raise _ffi.Yv3Error("yv3_cocoeval_workspace_bytes: invalid sizes")
    n_p, n_r = T * R * K * A * M, T * K * A * M
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    pinned = torch.from_numpy(buf).pin_memory()
    d_in = pinned.to(dev, non_blocking=True)
    ev[1].record()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(2 * n_p + n_r + 1, dtype=torch.float64, device=dev)
    base = d_in.data_ptr()
    p = [base + o for o in offs]
    d = _ffi.CocoEvalDesc()
    d.n_gt, d.n_det, d.n_img, d.n_cat = n_gt, n_det, int(n_img), K
    (d.gt_img, d.gt_cat, d.gt_box, d.gt_area, d.gt_crowd, d.gt_id, d.det_img, d.det_cat, d.det_box, d.det_score,
     d.iou_thrs, d.rec_thrs, d.area_rng) = p
    d.n_iou, d.n_rec, d.n_area, d.n_maxdet = T, R, A, M
    for i, m in enumerate(maxDets):
        d.max_dets[i] = m
    o = out.data_ptr()
    d.precision, d.scores, d.recall, d.status = o, o + 8 * n_p, o + 16 * n_p, o + 8 * (2 * n_p + n_r)
    _ffi.check(lib.yv3_cocoeval(d, ws.data_ptr(), ws_bytes, _ffi.stream_ptr()), "yv3_cocoeval")
    ev[2].record()
    res = out.cpu().numpy()
    ev[3].record()
    ev[3].synchronize()
    status = int(res[2 * n_p + n_r:].view(np.int32)[0])
    if status:
        _ffi.check(status, "yv3_cocoeval (more than 256 ground-truth boxes in one image for one category)")
    if timings is not None:
        timings.update(h2d=ev[0].elapsed_time(ev[1]) / 1e3, device=ev[1].elapsed_time(ev[2]) / 1e3,
                       d2h=ev[2].elapsed_time(ev[3]) / 1e3)
    return {'precision': res[:n_p].reshape(T, R, K, A, M).copy(), 'scores': res[n_p:2 * n_p].reshape(T, R, K, A, M).copy(),
            'recall': res[2 * n_p:2 * n_p + n_r].reshape(T, K, A, M).copy()}


def summarize_stats(ev, params, out=print):
    """pycocotools COCOeval.summarize (detections): the 12 statistics, each line printed in pycocotools' format."""
    p = params

    def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
        iStr = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        titleStr = 'Average Precision' if ap == 1 else 'Average Recall'
        typeStr = '(AP)' if ap == 1 else '(AR)'
        iouStr = '{:0.2f}:{:0.2f}'.format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
        aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
        if ap == 1:
            s = ev['precision']
            if iouThr is not None:
                s = s[np.where(iouThr == p.iouThrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = ev['recall']
            if iouThr is not None:
                s = s[np.where(iouThr == p.iouThrs)[0]]
            s = s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        if out is not None:
            out(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
        return mean_s

    stats = np.zeros((12,))
    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iouThr=.5, maxDets=p.maxDets[2])
    stats[2] = _summarize(1, iouThr=.75, maxDets=p.maxDets[2])
    stats[3] = _summarize(1, areaRng='small', maxDets=p.maxDets[2])
    stats[4] = _summarize(1, areaRng='medium', maxDets=p.maxDets[2])
    stats[5] = _summarize(1, areaRng='large', maxDets=p.maxDets[2])
    stats[6] = _summarize(0, maxDets=p.maxDets[0])
    stats[7] = _summarize(0, maxDets=p.maxDets[1])
    stats[8] = _summarize(0, maxDets=p.maxDets[2])
    stats[9] = _summarize(0, areaRng='small', maxDets=p.maxDets[2])
    stats[10] = _summarize(0, areaRng='medium', maxDets=p.maxDets[2])
    stats[11] = _summarize(0, areaRng='large', maxDets=p.maxDets[2])
    return stats


class COCOeval:
    """pycocotools.cocoeval.COCOeval for iouType 'bbox' (useCats = 1): ``params``, ``evaluate``, ``accumulate``,
    ``summarize``, ``stats``, ``eval``."""

    def __init__(self, cocoGt=None, cocoDt=None, iouType='bbox'):
        if iouType != 'bbox':
            raise NotImplementedError("only iouType 'bbox' is supported (segm / keypoints are not)")
        self.cocoGt, self.cocoDt = cocoGt, cocoDt
        self.params = Params(iouType=iouType)
        self.eval = {}
        self.stats = []
        self._result = None
        self.timings = {}
        if cocoGt is not None:
            self.params.imgIds = sorted(cocoGt.getImgIds())
            self.params.catIds = sorted(cocoGt.getCatIds())

    @property
    def evalImgs(self):
        raise NotImplementedError("per-image evaluation records are not kept: matching runs on the GPU")

    def _arrays(self):
        p = self.params
        img_keys = np.asarray(p.imgIds, dtype=np.int64)
        cat_keys = np.asarray(p.catIds, dtype=np.int64)
        gts = self.cocoGt.dataset.get('annotations', [])
        dts = self.cocoDt.dataset.get('annotations', [])
        ids = [g['id'] for g in gts]
        gt_img = _dense([g['image_id'] for g in gts], img_keys)
        gt_cat = _dense([g['category_id'] for g in gts], cat_keys)
        sel = (gt_img >= 0) & (gt_cat >= 0)
        if len(set(np.asarray(ids, dtype=np.int64)[sel].tolist())) != int(sel.sum()):
            raise ValueError("ground-truth annotation ids must be unique")
        return dict(
            gt_img=gt_img, gt_cat=gt_cat,
            gt_box=np.array([g['bbox'] for g in gts], dtype=np.float64).reshape(-1, 4),
            gt_area=np.array([g['area'] for g in gts], dtype=np.float64),
            gt_crowd=np.array([1 if g.get('iscrowd', 0) else 0 for g in gts], dtype=np.int32),
            gt_id=np.array(ids, dtype=np.int64),
            det_img=_dense([d['image_id'] for d in dts], img_keys), det_cat=_dense([d['category_id'] for d in dts], cat_keys),
            det_box=np.array([d['bbox'] for d in dts], dtype=np.float64).reshape(-1, 4),
            det_score=np.array([d['score'] for d in dts], dtype=np.float64))

    def evaluate(self):
        tic = time.time()
        print('Running per image evaluation...')
        p = self.params
        if p.useCats != 1:
            raise NotImplementedError("useCats = 0 is not supported")
        if p.iouType != 'bbox':
            raise NotImplementedError("only iouType 'bbox' is supported")
        print('Evaluate annotation type *{}*'.format(p.iouType))
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        self.params = p
        self._paramsEval = copy.deepcopy(p)
        t0 = time.time()
        arrays = self._arrays()
        self.timings['map'] = time.time() - t0
        self._result = run_device(n_img=max(len(p.imgIds), 1), n_cat=max(len(p.catIds), 1), iouThrs=p.iouThrs, recThrs=p.recThrs,
                                  areaRng=p.areaRng, maxDets=p.maxDets, timings=self.timings, **arrays)
        if not p.catIds:                                         # (no categories: empty arrays, as pycocotools gives)
            self._result = {k: v[:, :, :0] if k != 'recall' else v[:, :0] for k, v in self._result.items()}
        print('DONE (t={:0.2f}s).'.format(time.time() - tic))

    def accumulate(self, p=None):
        if self._result is None:
            raise Exception('Please run evaluate() first')
        if p is not None and p is not self.params:
            raise NotImplementedError("accumulate(p) with other parameters is not supported: set params before evaluate()")
        tic = time.time()
        print('Accumulating evaluation results...')
        p = self.params
        T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        self.eval = {'params': p, 'counts': [T, R, K, A, M], 'date': time.strftime('%Y-%m-%d %H:%M:%S'),
                     'precision': self._result['precision'], 'recall': self._result['recall'], 'scores': self._result['scores']}
        print('DONE (t={:0.2f}s).'.format(time.time() - tic))

    def summarize(self):
        if not self.eval:
            raise Exception('Please run accumulate() first')
        self.stats = summarize_stats(self.eval, self.params)

    def __str__(self):
        self.summarize()
        return ''


def detections_as_arrays(preds, gts):
    """Per-image ``detect()`` outputs and ground-truth boxes as the dense arrays of `run_device` (image index = list position,
    category = class index, GT ids 1, 2, ... so that none is 0).

    preds[i]: [n, 7] (x1, y1, x2, y2, conf, score, cls) or empty; the score is column 5, as in the results writer.
    gts[i]:   [m, 5] (x1, y1, x2, y2, cls), or a [m, 7] ``detect()`` output (class in column 6); crowd 0, area = w * h.
    Boxes become float64 xywh: x = x1, w = x2 - x1."""
    def rows(t, ncol):
        a = t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
        return a.reshape(-1, a.shape[-1] if a.size else ncol)

    g_img, g_rows, d_img, d_rows = [], [], [], []
    for i, (p, g) in enumerate(zip(preds, gts)):
        p, g = rows(p, 7), rows(g, 5)
        if len(p):
            d_img.append(np.full(len(p), i, np.int32))
            d_rows.append(p[:, [0, 1, 2, 3, 5, 6]])
        if len(g):
            g_img.append(np.full(len(g), i, np.int32))
            g_rows.append(g[:, [0, 1, 2, 3, 6 if g.shape[1] >= 7 else 4]])
    g = np.concatenate(g_rows) if g_rows else np.zeros((0, 5))
    d = np.concatenate(d_rows) if d_rows else np.zeros((0, 6))
    gbox = np.stack((g[:, 0], g[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]), 1)
    dbox = np.stack((d[:, 0], d[:, 1], d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]), 1)
    return dict(gt_img=np.concatenate(g_img) if g_img else np.zeros(0, np.int32), gt_cat=g[:, 4].astype(np.int32), gt_box=gbox,
                gt_area=gbox[:, 2] * gbox[:, 3], gt_crowd=np.zeros(len(g), np.int32), gt_id=np.arange(1, len(g) + 1, dtype=np.int64),
                det_img=np.concatenate(d_img) if d_img else np.zeros(0, np.int32), det_cat=d[:, 5].astype(np.int32), det_box=dbox,
                det_score=d[:, 4].copy())


def evaluate_detections(preds, gts, num_classes=80, iouThrs=None, recThrs=None, maxDets=None, areaRng=None, verbose=False):
    """COCO bbox evaluation of per-image ``detect()`` outputs against per-image ground-truth boxes (see
    `detections_as_arrays`), without files: images 0..len(preds)-1, categories 0..num_classes-1.  Returns ``{'precision',
    'recall', 'scores', 'stats', 'params'}`` with COCOeval's shapes and defaults."""
    if len(preds) != len(gts):
        raise ValueError("preds and gts must hold one entry per image")
    p = Params()
    p.imgIds, p.catIds = list(range(len(preds))), list(range(num_classes))
    if iouThrs is not None:
        p.iouThrs = np.asarray(iouThrs, dtype=np.float64)
    if recThrs is not None:
        p.recThrs = np.asarray(recThrs, dtype=np.float64)
    if maxDets is not None:
        p.maxDets = sorted(maxDets)
    if areaRng is not None:
        p.areaRng = areaRng
    arrays = detections_as_arrays(preds, gts)
    bad = (arrays['gt_cat'] < 0) | (arrays['gt_cat'] >= num_classes)
    arrays['gt_cat'] = np.where(bad, -1, arrays['gt_cat']).astype(np.int32)
    bad = (arrays['det_cat'] < 0) | (arrays['det_cat'] >= num_classes)
    arrays['det_cat'] = np.where(bad, -1, arrays['det_cat']).astype(np.int32)
    res = run_device(n_img=max(len(preds), 1), n_cat=num_classes, iouThrs=p.iouThrs, recThrs=p.recThrs, areaRng=p.areaRng,
                     maxDets=p.maxDets, **arrays)
    res['stats'] = summarize_stats(res, p, out=print if verbose else None)
    res['params'] = p
    return res
