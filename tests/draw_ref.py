"""The pixel rule of `yolo_v3_amd.draw.draw_boxes` in numpy (plain Python, no GPU): boxes painted one after the other into a copy
of the image, outline then tag, so that a later box covers an earlier one."""
import numpy as np


def draw(image, rects, colors, tags=None, masks=(), thickness=2):
    """``image``: uint8 ``[H, W, 3]``; ``rects``: int rows ``x1, y1, x2, y2``; ``colors``: uint8 rows; ``tags``: indices into
    ``masks`` (bool ``[mh, mw]`` arrays), -1 or ``tags=None`` for no tag.  Returns the painted copy.

    Outline of a box: the pixels of ``[x1, x2] x [y1, y2]`` (both ends included) less than ``thickness`` pixels away from one of
    the four sides, clipped to the image.  Tag of size ``(mw, mh)``: left edge at ``clip(x1, 0, W - mw)``, bottom edge (exclusive)
    at ``clip(y1, mh, H)`` -- the reference's ``cv2_drawTextWithBkgd`` placement; a negative left edge becomes 0, and what lies
    outside the image is cropped.  The tag is filled with the box colour, black where the mask is set."""
    out = np.array(image, dtype=np.uint8, copy=True)
    H, W = out.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    t = int(thickness)
    for j, (x1, y1, x2, y2) in enumerate(np.asarray(rects, dtype=np.int64).reshape(-1, 4)):
        color = np.asarray(colors[j], dtype=np.uint8)
        inside = (xs >= x1) & (xs <= x2) & (ys >= y1) & (ys <= y2)
        near = (xs - x1 < t) | (x2 - xs < t) | (ys - y1 < t) | (y2 - ys < t)
        out[inside & near] = color
        tag = -1 if tags is None else int(tags[j])
        if tag < 0:
            continue
        mask = np.asarray(masks[tag], dtype=bool)
        mh, mw = mask.shape
        left = max(int(np.clip(x1, 0, W - mw)), 0)                 # (np.clip with W - mw < 0 gives W - mw)
        bottom = int(np.clip(y1, mh, H))
        top = bottom - mh
        for y in range(max(top, 0), min(bottom, H)):
            for x in range(left, min(left + mw, W)):
                out[y, x] = 0 if mask[y - top, x - left] else color
    return out
