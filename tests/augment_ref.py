"""Numpy restatement of the training augmentation (yolo_v3_amd/augment.py, csrc/augment.hip) for the tests: the reference's
``Compose([IaaAugmentations([iaa_hsv_aug, iaa_random_crop, iaa.Fliplr, IaaLetterbox(dim)]), ToTensor()])`` with the random
draws given as parameters (dhue, dsat, dexp, top, right, bottom, left, flip).  Pixels: OpenCV's 8-bit RGB2HSV / HSV2RGB, then
the intermediate image is built explicitly (pad / crop, flip) and resized with oracle_cpu.cv_resize_cubic_u8.  Labels: float64,
step by step as transforms.py / imgaug do them (see the docstrings)."""
import numpy as np

from oracle import oracle_cpu as oc

F32_EPS = np.finfo(np.float32).eps


def _tables():
    i = np.arange(256, dtype=np.float64)
    with np.errstate(divide="ignore"):
        sdiv = np.where(i > 0, np.rint((255 << 12) / np.maximum(i, 1)), 0).astype(np.int64)
        hdiv = np.where(i > 0, np.rint((180 << 12) / (6.0 * np.maximum(i, 1))), 0).astype(np.int64)
    return sdiv, hdiv


SDIV, HDIV = _tables()


def rgb2hsv_u8(img):
    """cv2.cvtColor(img, COLOR_RGB2HSV) for uint8 [..., 3] (RGB2HSV_b: hsv_shift 12, hue range 180)."""
    x = img.astype(np.int64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    vr = np.where(v == r, -1, 0)
    vg = np.where(v == g, -1, 0)
    s = (diff * SDIV[v] + (1 << 11)) >> 12
    h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + (~vg & (r - g + 4 * diff))))
    h = (h * HDIV[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return np.stack([h, s, v], -1).astype(np.uint8)


def hsv2rgb_u8(hsv):
    """cv2.cvtColor(hsv, COLOR_HSV2RGB) for uint8 [..., 3] (HSV2RGB_b: float32 h * (6/180) wrapped into [0, 6), s and v times
    1/255, the sector table, saturate_cast<uchar>(x * 255))."""
    f32 = np.float32
    h = hsv[..., 0].astype(f32)
    s = hsv[..., 1].astype(f32) * f32(1.0 / 255.0)
    v = hsv[..., 2].astype(f32) * f32(1.0 / 255.0)
    h = h * (f32(6.0) / f32(180.0))
    h = np.where(h >= f32(6.0), h - f32(6.0), h).astype(f32)
    sector = np.floor(h).astype(np.int64)
    h = (h - sector.astype(f32)).astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, f32(0.0), h).astype(f32)
    one = f32(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], -1).astype(f32)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])        # (b, g, r) per sector
    idx = sd[sector]
    bgr = np.take_along_axis(tab, idx, -1)
    grey = (s == 0)[..., None]
    bgr = np.where(grey, v[..., None], bgr)
    rgb = bgr[..., ::-1]
    return np.clip(np.rint(rgb * f32(255.0)), 0, 255).astype(np.uint8)


def hsv_jitter(img, dhue, dsat, dexp):
    """Step 1 (iaa_hsv_aug): RGB2HSV, h + dhue, s * dsat, v * dexp in float32 clipped to [0, 255] and truncated, HSV2RGB."""
    f32 = np.float32
    hsv = rgb2hsv_u8(img)
    h = np.clip(hsv[..., 0].astype(f32) + f32(dhue), 0, 255).astype(np.uint8)
    s = np.clip(hsv[..., 1].astype(f32) * f32(dsat), 0, 255).astype(np.uint8)
    v = np.clip(hsv[..., 2].astype(f32) * f32(dexp), 0, 255).astype(np.uint8)
    return hsv2rgb_u8(np.stack([h, s, v], -1))


def hsv_roundtrip(img):
    return hsv_jitter(img, 0.0, 1.0, 1.0)


def crop_pad_flip(img, top, right, bottom, left, flip):
    """Steps 2-3: CropAndPad(px=(top, right, bottom, left), keep_size=False, pad_cval=128), then Fliplr when flip."""
    H, W = img.shape[:2]
    top, right, bottom, left = int(top), int(right), int(bottom), int(left)
    H1, W1 = H + top + bottom, W + left + right
    out = np.full((H1, W1, 3), 128, dtype=np.uint8)
    ys, xs = max(0, -top), max(0, -left)                       # first source row / column kept
    ye, xe = min(H, H1 - top), min(W, W1 - left)
    if ye > ys and xe > xs:
        out[ys + top:ye + top, xs + left:xe + left] = img[ys:ye, xs:xe]
    if flip:
        out = out[:, ::-1].copy()
    return out


def intermediate(img, p):
    """The image IaaLetterbox receives: steps 1-3 of one image with parameters p."""
    return crop_pad_flip(hsv_jitter(img, p[0], p[1], p[2]), p[3], p[4], p[5], p[6], p[7])


def letterbox_u8(img1, dim):
    """Step 4 before ToTensor: IaaLetterbox(dim) of the intermediate, uint8 [h, w, 3]."""
    H1, W1 = img1.shape[:2]
    rw, rh, xp, yp = oc.iaa_letterbox_params(img1.shape, dim[1], dim[0])
    canvas = np.full((dim[1], dim[0], 3), 128, dtype=np.uint8)
    canvas[yp:yp + rh, xp:xp + rw] = oc.cv_resize_cubic_u8(img1, rw, rh)
    return canvas


def augment_image_u8(img, p, dim):
    """The canvas bytes of one image: uint8 [h, w, 3] (ToTensor divides them by 255)."""
    return letterbox_u8(intermediate(img, p), dim)


def augment_image(img, p, dim):
    """ToTensor of the canvas: float32 [3, h, w]."""
    return (augment_image_u8(img, p, dim).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)


# ---- labels -------------------------------------------------------------------------------------------------------------------
def cxcywh_rel_to_xyxy_abs(rows, W, H):
    """BoundingBoxConverter.convert(Relative cxcywh -> Absolute x1y1x2y2): the format first, then the coordinates."""
    b = np.array(rows, dtype=np.float64).reshape(-1, 5).copy()
    cx, cy, w, h = b[:, 1].copy(), b[:, 2].copy(), b[:, 3].copy(), b[:, 4].copy()
    b[:, 1], b[:, 3] = cx - w / 2, cx + w / 2
    b[:, 2], b[:, 4] = cy - h / 2, cy + h / 2
    b[:, [1, 3]] *= W
    b[:, [2, 4]] *= H
    return b


def xyxy_abs_to_cxcywh_rel(rows, W, H):
    """BoundingBoxConverter.convert(Absolute x1y1x2y2 -> Relative cxcywh)."""
    b = np.array(rows, dtype=np.float64).reshape(-1, 5).copy()
    bw, bh = b[:, 3] - b[:, 1], b[:, 4] - b[:, 2]
    b[:, 1], b[:, 2], b[:, 3], b[:, 4] = b[:, 1] + bw / 2, b[:, 2] + bh / 2, bw, bh
    b[:, [1, 3]] /= W
    b[:, [2, 4]] /= H
    return b


def clip_keep(x1, y1, x2, y2, width, height, area_thr=0.1):
    """bbs_clip (transforms.py:241-259) of one box on a (height, width) image: (keep, (clipped box), kept-area fraction).
    ``width - eps`` is a float32 scalar operation there (python int - np.float32)."""
    xm = float(np.float32(width) - F32_EPS)
    ym = float(np.float32(height) - F32_EPS)
    c1, c2 = min(max(x1, 0.0), xm), min(max(x2, 0.0), xm)
    d1, d2 = min(max(y1, 0.0), ym), min(max(y2, 0.0), ym)
    frac = (c2 - c1) * (d2 - d1) / ((y2 - y1) * (x2 - x1))
    return frac > area_thr, (c1, d1, c2, d2), frac


def augment_labels(rows, H, W, p, dim, max_labels=90, with_fracs=False):
    """Label side of the transform for one image: [max_labels, 5] float64 (cls, cx, cy, w, h relative to dim), zero-filled.
    ``with_fracs``: also the kept-area fraction of every row that reaches bbs_remove_cut_out (to keep tests off the threshold)."""
    top, right, bottom, left, flip = int(p[3]), int(p[4]), int(p[5]), int(p[6]), p[7] != 0
    H1, W1 = H + top + bottom, W + left + right
    rw, rh, xp, yp = oc.iaa_letterbox_params((H1, W1), dim[1], dim[0])
    kept, fracs = [], []
    for r in cxcywh_rel_to_xyxy_abs(rows, W, H):
        cls, x1, y1, x2, y2 = (float(v) for v in r)
        if not (x2 > x1 and y2 > y1):                            # label_np_to_bbs
            continue
        x1, x2, y1, y2 = x1 + left, x2 + left, y1 + top, y2 + top
        if flip:
            x1, x2 = (W1 - 1) - x2, (W1 - 1) - x1
        x1, x2 = x1 * rw / W1 + xp, x2 * rw / W1 + xp
        y1, y2 = y1 * rh / H1 + yp, y2 * rh / H1 + yp
        keep, (x1, y1, x2, y2), frac = clip_keep(x1, y1, x2, y2, dim[0], dim[1])
        fracs.append(frac)
        if keep:
            kept.append((cls, x1, y1, x2, y2))
    out = np.zeros((max_labels, 5), dtype=np.float64)
    if kept:
        rel = xyxy_abs_to_cxcywh_rel(kept, dim[0], dim[1])[:max_labels]
        out[:len(rel)] = rel
    return (out, fracs) if with_fracs else out
