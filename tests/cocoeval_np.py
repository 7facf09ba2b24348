"""Plain float64 numpy restatement of COCO bbox evaluation (pycocotools 2.0.x semantics, iouType 'bbox', useCats 1).

Test infrastructure: written from the semantics list of the COCO-eval design ("COCO bbox mAP"), one step per
item, deliberately loop-shaped and slow.  ``evaluate(gt_dataset, results, ...)`` returns the arrays ``precision`` [T,R,K,A,M],
``recall`` [T,K,A,M], ``scores`` [T,R,K,A,M] and the 12 ``stats``.
"""
from collections import defaultdict

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']


def load_res(gt_dataset, results):
    """loadRes: det id = position + 1, area = w*h, iscrowd = 0; every image must be a GT image."""
    gt_imgs = set(im['id'] for im in gt_dataset['images'])
    anns = []
    for i, r in enumerate(results):
        if r['image_id'] not in gt_imgs:
            raise AssertionError('Results do not correspond to current coco set')
        bb = r['bbox']
        anns.append({'id': i + 1, 'image_id': r['image_id'], 'category_id': r['category_id'], 'bbox': list(bb),
                     'score': r['score'], 'area': bb[2] * bb[3], 'iscrowd': 0})
    return anns


def bb_iou(d, g, crowd):
    """maskApi bbIou, float64."""
    da = d[2] * d[3]
    ga = g[2] * g[3]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def evaluate(gt_dataset, results, imgIds=None, catIds=None, iouThrs=None, recThrs=None, maxDets=None, areaRng=None):
    iouThrs = IOU_THRS if iouThrs is None else np.asarray(iouThrs, dtype=np.float64)
    recThrs = REC_THRS if recThrs is None else np.asarray(recThrs, dtype=np.float64)
    maxDets = sorted(MAX_DETS if maxDets is None else maxDets)
    areaRng = AREA_RNG if areaRng is None else areaRng
    imgIds = sorted(set(im['id'] for im in gt_dataset['images'])) if imgIds is None else list(np.unique(imgIds))
    catIds = sorted(set(c['id'] for c in gt_dataset['categories'])) if catIds is None else list(np.unique(catIds))
    dts_all = load_res(gt_dataset, results)
    setI, setK = set(imgIds), set(catIds)

    # _prepare: groups keyed (image, category), file order kept; ignore = iscrowd
    gts, dts = defaultdict(list), defaultdict(list)
    for g in gt_dataset['annotations']:
        if g['image_id'] in setI and g['category_id'] in setK:
            g = dict(g)
            g['ignore'] = bool(g.get('iscrowd', 0))
            gts[g['image_id'], g['category_id']].append(g)
    for d in dts_all:
        if d['image_id'] in setI and d['category_id'] in setK:
            dts[d['image_id'], d['category_id']].append(d)

    T, R, K, A, M = len(iouThrs), len(recThrs), len(catIds), len(areaRng), len(maxDets)
    maxDet = maxDets[-1]

    def evaluate_img(imgId, catId, aRng):
        gt, dt = gts[imgId, catId], dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        gig = [1 if (g['ignore'] or g['area'] < aRng[0] or g['area'] > aRng[1]) else 0 for g in gt]
        gtind = np.argsort(gig, kind='mergesort')
        gt = [gt[i] for i in gtind]
        gtIg = np.array([gig[i] for i in gtind])
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[0:maxDet]]
        crowd = [int(g['iscrowd']) for g in gt]
        G, D = len(gt), len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        dtIg = np.zeros((T, D))
        if G and D:
            ious = np.array([[bb_iou(d['bbox'], g['bbox'], crowd[j]) for j, g in enumerate(gt)] for d in dt])
            for tind, t in enumerate(iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind in range(G):
                        if gtm[tind, gind] > 0 and not crowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        out_of_area = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, D))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(out_of_area, T, 0)))
        return {'dtScores': np.array([d['score'] for d in dt], dtype=np.float64), 'dtMatches': dtm, 'dtIgnore': dtIg,
                'gtIgnore': gtIg}

    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k, catId in enumerate(catIds):
        for a, aRng in enumerate(areaRng):
            E = [evaluate_img(i, catId, aRng) for i in imgIds]
            E = [e for e in E if e is not None]
            if not E:
                continue
            for m, md in enumerate(maxDets):
                dtScores = np.concatenate([e['dtScores'][0:md] for e in E])
                inds = np.argsort(-dtScores, kind='mergesort')
                dtScoresSorted = dtScores[inds]
                dtm = np.concatenate([e['dtMatches'][:, 0:md] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e['dtIgnore'][:, 0:md] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e['gtIgnore'] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    pis = np.searchsorted(rc, recThrs, side='left')
                    for ri, pi in enumerate(pis):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                        ss[ri] = dtScoresSorted[pi]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    out = {'precision': precision, 'recall': recall, 'scores': scores}
    out['stats'] = summarize(out, iouThrs, maxDets, AREA_LBL[:len(areaRng)])
    return out


def summarize(ev, iouThrs, maxDets, areaRngLbl):
    def one(ap=1, iouThr=None, areaRng='all', maxDets_=100):
        aind = [i for i, lbl in enumerate(areaRngLbl) if lbl == areaRng]
        mind = [i for i, md in enumerate(maxDets) if md == maxDets_]
        if ap == 1:
            s = ev['precision']
            if iouThr is not None:
                s = s[np.where(iouThr == iouThrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = ev['recall']
            if iouThr is not None:
                s = s[np.where(iouThr == iouThrs)[0]]
            s = s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    st = np.zeros((12,))
    st[0] = one(1)
    st[1] = one(1, iouThr=.5, maxDets_=maxDets[2])
    st[2] = one(1, iouThr=.75, maxDets_=maxDets[2])
    st[3] = one(1, areaRng='small', maxDets_=maxDets[2])
    st[4] = one(1, areaRng='medium', maxDets_=maxDets[2])
    st[5] = one(1, areaRng='large', maxDets_=maxDets[2])
    st[6] = one(0, maxDets_=maxDets[0])
    st[7] = one(0, maxDets_=maxDets[1])
    st[8] = one(0, maxDets_=maxDets[2])
    st[9] = one(0, areaRng='small', maxDets_=maxDets[2])
    st[10] = one(0, areaRng='medium', maxDets_=maxDets[2])
    st[11] = one(0, areaRng='large', maxDets_=maxDets[2])
    return st


def synthetic_set(seed, n_img=24, n_cat=12, gt_per_img=8, det_per_img=24, id0=False, crowd=True, big_group=False,
                  id_base=100):
    """A seeded COCO ground truth + results pair from ``synth.uniform`` turned into integers: sparse image ids, integer box
    corners (so areas hit 32^2 / 96^2 exactly and zero-width boxes occur), scores on a 1/16 grid (ties inside and across
    images), crowd GTs, categories with dets but no GT, images with GT but no dets; ``id0``: annotation ids from 0;
    ``big_group``: one (image, category) group with 130 dets."""
    from yolo_v3_amd import synth

    def ints(stream, n, lo, hi):                  # integers in [lo, hi)
        return np.floor(synth.uniform(seed, stream, n, lo, hi)).astype(np.int64)

    img_ids = sorted(set((id_base + 7 * np.arange(n_img) + ints(1, n_img, 0, 5)).tolist()))
    n_img = len(img_ids)
    gt_cats = list(range(0, n_cat - 2))           # the last two categories never have a GT
    images = [{"id": int(i), "width": 640, "height": 480} for i in img_ids]
    cats = [{"id": c, "name": "c%d" % c} for c in range(n_cat)]
    anns, res = [], []
    special_wh = [(32, 32), (96, 96), (0, 40), (40, 0), (31, 33), (97, 95)]
    s = 10
    for ii, iid in enumerate(img_ids):
        ng = int(ints(s, 1, 0, gt_per_img + 1)[0]); s += 1
        xs, ys = ints(s, ng, 0, 560), ints(s + 1, ng, 0, 400); s += 2
        ws, hs = ints(s, ng, 1, 160), ints(s + 1, ng, 1, 140); s += 2
        cs = ints(s, ng, 0, len(gt_cats)); s += 1
        cr = ints(s, ng, 0, 20); s += 1
        boxes = []
        for j in range(ng):
            w, h = int(ws[j]), int(hs[j])
            if j < len(special_wh) and ii % 3 == 0:
                w, h = special_wh[j]
            iscrowd = 1 if (crowd and cr[j] == 0) else 0
            anns.append({"id": len(anns) + (0 if id0 else 1), "image_id": int(iid), "category_id": int(gt_cats[cs[j]]),
                         "iscrowd": iscrowd, "area": float(w * h), "bbox": [float(xs[j]), float(ys[j]), float(w), float(h)]})
            boxes.append((float(xs[j]), float(ys[j]), float(w), float(h), int(gt_cats[cs[j]])))
        if ii % 5 == 4:                           # GT but no dets
            continue
        nd = int(ints(s, 1, 0, det_per_img + 1)[0]); s += 1
        sc = ints(s, nd, 0, 16); s += 1
        pick = ints(s, nd, 0, 4); s += 1
        jit = ints(s, 4 * nd, -6, 7).reshape(nd, 4); s += 1
        rx, ry, rw, rh = ints(s, nd, 0, 600), ints(s + 1, nd, 0, 440), ints(s + 2, nd, 0, 120), ints(s + 3, nd, 0, 120); s += 4
        rc = ints(s, nd, 0, n_cat); s += 1
        for j in range(nd):
            if boxes and pick[j] != 0:            # near a GT of the image (jittered corners)
                b = boxes[j % len(boxes)]
                x, y = b[0] + jit[j, 0], b[1] + jit[j, 1]
                w, h = max(0.0, b[2] + jit[j, 2]), max(0.0, b[3] + jit[j, 3])
                c = b[4]
            else:
                x, y, w, h, c = float(rx[j]), float(ry[j]), float(rw[j]), float(rh[j]), int(rc[j])
            res.append({"image_id": int(iid), "category_id": int(c), "bbox": [float(x), float(y), float(w), float(h)],
                        "score": float(sc[j] + 1) / 16.0})
        if big_group and ii == 1:
            for j in range(130):
                res.append({"image_id": int(iid), "category_id": 0, "bbox": [float(j % 50), float(j % 37), 40.0, 30.0],
                            "score": float(j % 13 + 1) / 16.0})
    return {"images": images, "categories": cats, "annotations": anns}, res
