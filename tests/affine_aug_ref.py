"""numpy restatement of the affine training augmentation (rotate, scale, shear, shift) as this project defines it: the yardstick
for csrc/affine_augment.hip and yolo_v3_amd/affine_augment.py, float64 throughout.  Deliberately slow and plain.

Geometry.  Continuous pixel coordinates: pixel (x, y) covers [x, x+1) x [y, y+1).  The output has the source's size (H, W).
``fwd`` (2x3, source -> output, used for labels) is ``T(C + t) . A . T(-C)`` with C = (W/2, H/2), t = (tx W, ty H) and
``A = [[s cos(th), -s sin(th + ph)], [s sin(th), s cos(th + ph)]]`` -- the linear part of skimage's AffineTransform(scale,
rotation, shear), which imgaug's Affine uses (recalled: neither library is installed where this was written).  ``inv`` (output ->
source, used for pixels) is the closed-form inverse of ``fwd``: adjugate over determinant.

Pixels (`warp_ref`).  What Pillow's ``Image.transform(size, Image.AFFINE, inv, resample=Image.BILINEAR, fillcolor=(128,) * 3)``
computes on an RGB image [pinned: tests/test_affine_aug_host.py, bit for bit].  For output pixel (x, y), no fused multiply-add:
    xin = inv0 (x + 0.5) + inv1 (y + 0.5) + inv2, summed left to right; yin likewise from inv3..5
    xin < 0 or xin >= W or yin < 0 or yin >= H: the pixel is (128, 128, 128)
    otherwise xin -= 0.5, yin -= 0.5, x0 = floor(xin), y0 = floor(yin), dx = xin - x0, dy = yin - y0;
      columns x0 and x0 + 1 are clamped to [0, W-1], row y0 to [0, H-1];
      v1 = p[y0, x0] + (p[y0, x1] - p[y0, x0]) dx;  v2 the same on row y0 + 1 when 0 <= y0 + 1 < H, else v2 = v1;
      the byte is trunc(v1 + (v2 - v1) dy).

Labels (`labels_ref`).  The reference's rule for any imgaug geometry (iaa_run_seq, bbs_remove_cut_out(., 0.1), bbs_clip;
transforms.py:214-259) [unpinned: imgaug's keypoint rule is recalled].  A row (cls, cx, cy, w, h) relative to the source with
w <= 0 or h <= 0 becomes a zero row; otherwise its absolute corners (BoundingBoxConverter.convert's operation order) go through
``fwd``, the axis-aligned hull of the four mapped corners is clipped to [0, W - eps] x [0, H - eps] (eps = float32's), the row
is kept iff clipped area / hull area > 0.1 (strictly; a hull area <= 0 drops it) and converted back to relative cx cy w h.  Kept
rows stay in place, dropped rows are zeros.

A program with ``active == 0`` (iaa.Sometimes not firing) copies the image and passes its label rows through untouched.
"""
import numpy as np

EPS = float(np.float64(np.finfo(np.float32).eps))


def matrices(H, W, theta=0.0, scale=1.0, shear=0.0, tx=0.0, ty=0.0):
    """``(fwd, inv)``, float64 ``[6]`` each: angles in radians, tx / ty fractions of W / H."""
    H, W = float(H), float(W)
    a = np.float64(scale) * np.cos(np.float64(theta))
    b = -np.float64(scale) * np.sin(np.float64(theta) + np.float64(shear))
    c = np.float64(scale) * np.sin(np.float64(theta))
    d = np.float64(scale) * np.cos(np.float64(theta) + np.float64(shear))
    cx, cy = np.float64(W / 2), np.float64(H / 2)
    ox, oy = cx + np.float64(tx) * W, cy + np.float64(ty) * H
    fwd = np.array([a, b, ox - (a * cx + b * cy), c, d, oy - (c * cx + d * cy)], dtype=np.float64)
    return fwd, invert(fwd)


def invert(fwd):
    """The closed-form inverse of a 2x3 affine map: adjugate over determinant, float64."""
    a, b, e, c, d, f = (np.float64(v) for v in fwd)
    det = a * d - b * c
    with np.errstate(all="ignore"):
        return np.array([d / det, -b / det, (b * f - d * e) / det, -c / det, a / det, (c * e - a * f) / det], dtype=np.float64)


def program(H, W, active=True, **kw):
    fwd, inv = matrices(H, W, **kw)
    return {"active": int(active), "fwd": fwd, "inv": inv}


def warp_ref(img, prog):
    """One uint8 ``[H,W,3]`` image through one program."""
    img = np.asarray(img)
    if not prog["active"]:
        return img.copy()
    H, W = img.shape[:2]
    inv = np.asarray(prog["inv"], dtype=np.float64)
    p = img.astype(np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    xc, yc = xx + 0.5, yy + 0.5
    xin = inv[0] * xc + inv[1] * yc + inv[2]
    yin = inv[3] * xc + inv[4] * yc + inv[5]
    outside = ~((xin >= 0) & (xin < W) & (yin >= 0) & (yin < H))
    xin, yin = np.where(outside, 0.5, xin) - 0.5, np.where(outside, 0.5, yin) - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    ya = np.clip(y0, 0, H - 1)
    v1 = p[ya, xa] + (p[ya, xb] - p[ya, xa]) * dx
    second = (y0 + 1 >= 0) & (y0 + 1 < H)
    yb = np.where(second, y0 + 1, ya)
    v2 = p[yb, xa] + (p[yb, xb] - p[yb, xa]) * dx
    v2 = np.where(second[..., None], v2, v1)
    v = v1 + (v2 - v1) * dy
    out = np.trunc(v).astype(np.uint8)
    out[outside] = 128
    return out


def labels_ref(rows, H, W, prog):
    """``[T,5]`` float64 rows of one image through one program -> ``[T,5]`` (kept rows in place, dropped rows zeros)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    if not prog["active"]:
        return rows.copy()
    f = np.asarray(prog["fwd"], dtype=np.float64)
    out = np.zeros_like(rows)
    Wd, Hd = np.float64(W), np.float64(H)
    xmax, ymax = Wd - EPS, Hd - EPS
    for i, (cls, cx, cy, w, h) in enumerate(rows):
        if w <= 0 or h <= 0:
            continue
        x1, x2 = (cx - w / 2) * Wd, (cx + w / 2) * Wd
        y1, y2 = (cy - h / 2) * Hd, (cy + h / 2) * Hd
        xs, ys = [], []
        for x, y in ((x1, y1), (x2, y1), (x2, y2), (x1, y2)):
            xs.append(f[0] * x + f[1] * y + f[2])
            ys.append(f[3] * x + f[4] * y + f[5])
        hx1, hx2 = min(min(xs[0], xs[1]), min(xs[2], xs[3])), max(max(xs[0], xs[1]), max(xs[2], xs[3]))
        hy1, hy2 = min(min(ys[0], ys[1]), min(ys[2], ys[3])), max(max(ys[0], ys[1]), max(ys[2], ys[3]))
        area = (hy2 - hy1) * (hx2 - hx1)
        if not area > 0:
            continue
        c1, c2 = min(max(hx1, 0.0), xmax), min(max(hx2, 0.0), xmax)
        d1, d2 = min(max(hy1, 0.0), ymax), min(max(hy2, 0.0), ymax)
        if not (c2 - c1) * (d2 - d1) / area > 0.1:
            continue
        bw, bh = c2 - c1, d2 - d1
        out[i] = (cls, (c1 + bw / 2) / Wd, (d1 + bh / 2) / Hd, bw / Wd, bh / Hd)
    return out


def affine_ref(images, labels, programs):
    """A batch: ``(images_out, labels_out)``, lists of uint8 ``[H,W,3]`` and float64 ``[n_i,5]``."""
    out_i = [warp_ref(im, p) for im, p in zip(images, programs)]
    out_l = [labels_ref(l, im.shape[0], im.shape[1], p) for im, l, p in zip(images, labels, programs)]
    return out_i, out_l
