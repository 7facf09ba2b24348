"""The host half the batched augmentation stages share (``augment_batch``, ``extra_augment_batch``, ``affine_augment_batch``):
validating the images, padding the labels, and staging one batch -- a stage's per-image records, the images' offsets and shapes,
host labels and host images -- through a pinned buffer in one upload.

    staged buffer:  records | offsets | hw | labels | [gather: source offsets] or [images]        every section 256-aligned

``offsets`` are the images' 256-aligned positions in a packed batch of ``span`` bytes: where a packed source lies behind
``o_img``, and where a stage that returns images writes its outputs.  The *gather* path: when every image is a contiguous view
into one allocation on the current GPU (``TrainBatches``' arena, or the output of the stage before), no pixel is copied; the
images' offsets in that allocation are uploaded instead and the kernels read them where they are.
"""
import collections

import numpy as np
import torch

from . import _ffi

ALIGN = 256
counters = {"batches": 0, "upload_bytes": 0}     # augment_batch calls; the bytes every stage (and the loader's arena) uploads


def round_up(n, a=ALIGN):
    return (n + a - 1) // a * a


class _Staging:
    """Pinned host buffers for a stage's one upload, used in turn.  A buffer is rewritten only after the copy that last read
    it has completed: waiting for that copy's event is the path's only host synchronisation."""

    def __init__(self, n=2):
        self.bufs, self.events, self.i = [None] * n, [None] * n, 0

    def take(self, nbytes):
        i = self.i
        self.i = (i + 1) % len(self.bufs)
        if self.events[i] is not None:
            self.events[i].synchronize()
            self.events[i] = None
        if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
            self.bufs[i] = None
            self.bufs[i] = torch.empty(max(1 << 20, 1 << (nbytes - 1).bit_length()), dtype=torch.uint8, pin_memory=True)
        return i, self.bufs[i]

    def release(self, i):
        ev = torch.cuda.Event()
        ev.record()
        self.events[i] = ev


_staging = {}                # device index -> the pool all stages share


def as_images(images):
    """``(tensors, shapes)`` of a batch of uint8 RGB ``[H,W,3]`` numpy arrays or tensors (CPU or GPU): numpy arrays become CPU
    tensors, ``shapes`` are the ``(H, W)``."""
    if not torch.cuda.is_available():
        raise _ffi.Yv3Error("no GPU available: this package has no CPU path")
    imgs = []
    for img in images:
        t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise _ffi.Yv3Error("images must be uint8 [H,W,3] RGB")
        imgs.append(t)
    if not imgs:
        raise ValueError("empty batch")
    return imgs, [(int(t.shape[0]), int(t.shape[1])) for t in imgs]


def pad_labels(labels, B):
    """``(dev_labels, host_labels, T)`` of a batch's labels: a list of ``[n_i,5]`` arrays (n_i may be 0) becomes a zero-padded
    float64 ``[B,T,5]`` host array, a padded ``[B,T,5]`` tensor becomes float64 where it is (one of the two is None), None is
    ``T = 0``."""
    dev_labels, host_labels, T = None, None, 0
    if isinstance(labels, torch.Tensor):
        if labels.dim() != 3 or labels.shape[0] != B or labels.shape[2] != 5:
            raise ValueError("padded labels must be [B,T,5]")
        T = int(labels.shape[1])
        if labels.is_cuda:
            dev_labels = labels.to(torch.float64).contiguous()
        else:
            host_labels = labels.to(torch.float64).numpy()
    elif labels is not None:
        if len(labels) != B:
            raise ValueError("one label array per image")
        rows = [np.asarray(l, dtype=np.float64).reshape(-1, 5) for l in labels]
        T = max(r.shape[0] for r in rows)
        host_labels = np.zeros((B, T, 5), dtype=np.float64)
        for b, r in enumerate(rows):
            host_labels[b, :r.shape[0]] = r
    return dev_labels, host_labels, T


Layout = collections.namedtuple("Layout", "offsets span o_off o_hw o_lab o_img total upload")      # the records lie at 0


def layout(shapes, records_bytes, label_bytes, on_host, gather):
    """Where everything lies in the staged buffer -- integer arithmetic only.  ``shapes``: the images' ``(H, W)``;
    ``records_bytes`` / ``label_bytes``: the sizes of the two sections a stage fills (a stage without host labels has 0);
    ``on_host``: per image, whether its pixels come from the host; ``gather``: the gather path.  ``total`` bytes are allocated on
    the device and the first ``upload`` of them copied: everything when a host image is in the batch, the sections in front of
    the images when all are copied on the device, those and the source offsets when gathering."""
    B = len(shapes)
    offsets, pos = [], 0
    for H, W in shapes:
        offsets.append(pos)
        pos = round_up(pos + H * W * 3)
    o_off = round_up(records_bytes)
    o_hw = round_up(o_off + B * 8)
    o_lab = round_up(o_hw + B * 8)
    o_img = round_up(o_lab + label_bytes)
    if gather:
        total = upload = o_img + B * 8
    else:
        total = o_img + pos
        upload = total if any(on_host) else o_img
    return Layout(offsets, pos, o_off, o_hw, o_lab, o_img, total, upload)


def use_gather(imgs):
    """The gather path's condition: every image a contiguous view into one allocation on the current GPU."""
    dev_index = torch.cuda.current_device()
    return (all(t.is_cuda and t.device.index == dev_index and t.is_contiguous() for t in imgs)
            and len({t.untyped_storage().data_ptr() for t in imgs}) == 1)


# ``dev`` must stay referenced until the stage has enqueued its launches; the other fields are device pointers into it, but for
# ``offsets`` / ``span`` (host values) and, when ``gather``, ``src`` / ``src_bytes`` (the sources' own allocation)
Staged = collections.namedtuple("Staged", "dev offsets span gather records out_offsets hw labels src src_bytes src_offsets")


def stage_batch(imgs, shapes, records, host_labels=None):
    """Stage a batch on the current GPU and stream: ``records`` (a contiguous numpy array, the stage's per-image records,
    taken as bytes), the offsets, the shapes, ``host_labels`` (float64 ``[B,T,5]`` or None) and the host images go up in one copy
    from a pinned buffer, GPU images are copied on the device or gathered.  The kernels read image b at ``src + src_offsets[b]``
    (checked against ``src_bytes``); ``out_offsets`` is the device copy of ``offsets``."""
    B = len(imgs)
    gather = use_gather(imgs)
    records = records.reshape(-1).view(np.uint8)
    label_bytes = host_labels.nbytes if host_labels is not None else 0
    L = layout(shapes, records.nbytes, label_bytes, [not t.is_cuda for t in imgs], gather)
    o_img = L.o_img

    staging = _staging.setdefault(torch.cuda.current_device(), _Staging())
    slot, buf = staging.take(L.upload)
    host = buf.numpy()
    host[:records.nbytes] = records
    host[L.o_off:L.o_off + B * 8].view(np.int64)[:] = L.offsets
    host[L.o_hw:L.o_hw + B * 8].view(np.int32)[:] = np.asarray(shapes, dtype=np.int32).reshape(-1)
    if label_bytes:
        host[L.o_lab:L.o_lab + label_bytes].view(np.float64)[:] = host_labels.reshape(-1)
    if gather:
        arena = imgs[0].untyped_storage()
        host[o_img:o_img + B * 8].view(np.int64)[:] = [t.data_ptr() - arena.data_ptr() for t in imgs]
    for off, t in zip(L.offsets, imgs):
        if not t.is_cuda:
            host[o_img + off:o_img + off + t.numel()] = t.reshape(-1).numpy()
    dev = torch.empty(L.total, dtype=torch.uint8, device="cuda")
    dev[:L.upload].copy_(buf[:L.upload], non_blocking=True)
    staging.release(slot)
    counters["upload_bytes"] += L.upload
    if not gather:
        for off, t in zip(L.offsets, imgs):
            if t.is_cuda:
                dev[o_img + off:o_img + off + t.numel()].copy_(t.reshape(-1))

    base = dev.data_ptr()
    if gather:
        src, src_bytes, src_offsets = arena.data_ptr(), arena.nbytes(), base + o_img
    else:
        src, src_bytes, src_offsets = base + o_img, L.span, base + L.o_off
    return Staged(dev, L.offsets, L.span, gather, base, base + L.o_off, base + L.o_hw, base + L.o_lab, src, src_bytes, src_offsets)
