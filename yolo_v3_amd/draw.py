"""Box outlines and label tags drawn on the GPU into a batch of uint8 RGB images, in place (``csrc/draw.hip``, DESIGN.md section
8h) -- the stage between `detect` / ``yv3_correct_boxes`` and `jpeg.encode_batch` that keeps annotated frames on the device.

The kernel knows no font: `LabelAtlas` rasterises each class name once on the host (``ImageFont.load_default()`` /
``ImageDraw.text``) into a 1-bit mask.  The pixel rule (outline, tag placement as the reference's ``cv2_drawTextWithBkgd``, paint
order) is stated in include/yv3.h at ``yv3_draw_boxes`` and restated in numpy in tests/draw_ref.py."""
import ctypes

import numpy as np
import torch

from . import _ffi
from ._staging import round_up


def palette(n):
    """``n`` distinct RGB colours as uint8 ``[n, 3]``, a fixed rule: colour i spreads the bits of i + 1 over the three channels
    from the top bit down (the PASCAL VOC colour map without its black entry), distinct for n <= 255."""
    out = np.zeros((n, 3), np.uint8)
    for i in range(n):
        c, r, g, b = i + 1, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        out[i] = (r, g, b)
    return out


def rectangles(xywh):
    """Integer ``(x1, y1, x2, y2)`` rows, int32, of ``[n, 4]`` boxes ``x, y, w, h`` in image pixels: ``np.rint`` in float64 of the
    corners ``x, y, x + w, y + h`` (both corners belong to the rectangle)."""
    b = np.asarray(xywh, dtype=np.float64).reshape(-1, 4)
    corners = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1)
    return np.clip(np.rint(corners), -2 ** 30, 2 ** 30).astype(np.int32)


def rasterise(text, margin=1):
    """The 1-bit mask of ``text`` in PIL's default font: bool ``[mh, mw]``, True where there is ink, ``margin`` clear pixels around
    the text's box."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default()
    left, top, right, bottom = font.getbbox(text) if text else (0, 0, 0, 0)
    im = Image.new("1", (max(int(right), 0) + 16, max(int(bottom), 0) + 16), 0)       # room to spare; cropped to the ink below
    if text:
        ImageDraw.Draw(im).text((8, 8), text, fill=1, font=font)
    ink = np.asarray(im, dtype=bool)
    ys, xs = np.nonzero(ink)
    if len(ys) == 0:
        return np.zeros((1 + 2 * margin, 1 + 2 * margin), bool)
    return np.pad(ink[ys.min():ys.max() + 1, xs.min():xs.max() + 1], margin)


class LabelAtlas:
    """The masks of a list of class names, packed for the kernel: ``masks[i]`` is bool ``[mh, mw]``; ``data`` holds them back to
    back, each row in ``ceil(mw / 8)`` bytes with the leftmost pixel in bit 7 (``np.packbits``); ``records[i]`` = (byte offset,
    mw, mh).  The device copy is made once per device."""

    def __init__(self, names=(), masks=None):
        self.masks = [np.asarray(m, dtype=bool) for m in masks] if masks is not None else [rasterise(str(n)) for n in names]
        chunks, self.records, pos = [], [], 0
        for m in self.masks:
            assert m.ndim == 2 and m.shape[0] >= 1 and m.shape[1] >= 1
            packed = np.packbits(m, axis=1)
            self.records.append((pos, int(m.shape[1]), int(m.shape[0])))
            chunks.append(packed.reshape(-1))
            pos += packed.size
        self.data = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
        self._device = {}

    def __len__(self):
        return len(self.masks)

    def on(self, dev):
        """(tags tensor, atlas tensor) on ``dev``: the ``yv3_draw_tag`` records and the mask bytes."""
        if dev not in self._device:
            tags = (_ffi.DrawTag * max(len(self), 1))()
            for i, (off, mw, mh) in enumerate(self.records):
                tags[i] = _ffi.DrawTag(offset=off, width=mw, height=mh)
            t = torch.from_numpy(np.frombuffer(tags, dtype=np.uint8).copy()).to(dev)
            a = torch.from_numpy(self.data if self.data.size else np.zeros(1, np.uint8)).to(dev)
            self._device[dev] = (t, a)
        return self._device[dev]


def draw_boxes(images, rects, colors, tags=None, atlas=None, thickness=2):
    """Draw into ``images`` (uint8 ``[H,W,3]`` GPU tensors of any sizes, rows may be pitched) in place, one launch for the batch.
    ``rects[i]``: int ``[n_i, 4]`` rows ``x1, y1, x2, y2`` (`rectangles`); ``colors[i]``: uint8 ``[n_i, 3]``; ``tags[i]``: ``[n_i]``
    indices into ``atlas`` (a `LabelAtlas`), -1 for no tag; ``tags=None``: no tags at all.  Boxes paint in the order given, outline
    then tag, later boxes over earlier ones; an image without boxes is not written.  Returns ``images``."""
    if not torch.cuda.is_available():
        raise _ffi.Yv3Error("no GPU available: this package has no CPU path")
    images = list(images)
    B = len(images)
    if not (len(rects) == len(colors) == B) or (tags is not None and len(tags) != B):
        raise ValueError("draw_boxes: one list of rectangles, colours and tags per image")
    if int(thickness) < 1:
        raise ValueError("draw_boxes: thickness must be at least 1")
    if B == 0:
        return images
    dev = images[0].device
    recs = (_ffi.DrawImage * B)()
    boxes, first = [], 0
    for i, im in enumerate(images):
        _ffi.require_cuda(im, "images[%d]" % i)
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1 or im.device != dev:
            raise _ffi.Yv3Error("draw_boxes: images must be uint8 [H, W, 3] tensors on one GPU")
        if im.stride(2) != 1 or im.stride(1) != 3 or (im.shape[0] > 1 and im.stride(0) < 3 * im.shape[1]):
            raise _ffi.Yv3Error("draw_boxes: the pixels of a row must be contiguous (rows may be pitched)")
        r = np.asarray(rects[i], dtype=np.int32).reshape(-1, 4)
        c = np.asarray(colors[i], dtype=np.uint8).reshape(-1, 3)
        t = np.full(len(r), -1, np.int32) if tags is None else np.asarray(tags[i], dtype=np.int32).reshape(-1)
        if not (len(c) == len(t) == len(r)):
            raise ValueError("draw_boxes: image %d has %d rectangles, %d colours, %d tags" % (i, len(r), len(c), len(t)))
        if len(t) and t.max() >= (len(atlas) if atlas is not None else 0):
            raise ValueError("draw_boxes: image %d names a tag the atlas does not hold" % i)
        recs[i] = _ffi.DrawImage(pixels=im.data_ptr(), pitch=im.stride(0) if im.shape[0] > 1 else 3 * im.shape[1], width=im.shape[1],
                                 height=im.shape[0], first_box=first, num_boxes=len(r))
        for j in range(len(r)):
            boxes.append(_ffi.DrawBox(x1=int(r[j, 0]), y1=int(r[j, 1]), x2=int(r[j, 2]), y2=int(r[j, 3]), tag=int(t[j]),
                                      rgb=(ctypes.c_ubyte * 3)(*[int(v) for v in c[j]])))
        first += len(r)
    if first == 0:
        return images
    box_arr = (_ffi.DrawBox * first)(*boxes)
    n_img, n_box = ctypes.sizeof(recs), ctypes.sizeof(box_arr)
    o_box = round_up(n_img)
    with torch.cuda.device(dev):
        staging = torch.empty(o_box + n_box, dtype=torch.uint8, pin_memory=True)
        host = staging.numpy()
        host[:n_img] = np.frombuffer(recs, dtype=np.uint8)
        host[o_box:o_box + n_box] = np.frombuffer(box_arr, dtype=np.uint8)
        meta = staging.to(dev, non_blocking=True)
        tag_t, atlas_t = atlas.on(dev) if atlas is not None and len(atlas) else (None, None)
        _ffi.check(_ffi.lib().yv3_draw_boxes(meta.data_ptr(), B, meta.data_ptr() + o_box, first,
                                             tag_t.data_ptr() if tag_t is not None else None, len(atlas) if tag_t is not None else 0,
                                             atlas_t.data_ptr() if atlas_t is not None else None,
                                             atlas_t.numel() if atlas_t is not None else 0, int(thickness),
                                             max(im.shape[1] for im in images), max(im.shape[0] for im in images), _ffi.stream_ptr()),
                   "yv3_draw_boxes")
    return images
