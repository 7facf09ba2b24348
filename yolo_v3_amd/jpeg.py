"""JPEG decode on the GPU, bit for bit with PIL (libjpeg-turbo's defaults): ``csrc/jpeg_parse.cpp`` reads the headers on
the host, ``csrc/jpeg.hip`` decodes a batch of files in four launches, five when ``progressive=True``
and the batch holds a progressive file (section 8f.2).

``decode_batch(sources)`` returns what ``evaluate.read_image_rgb`` returns for every source, as GPU tensors.  A file the parser
does not positively recognise (progressive unless ``progressive=True``, arithmetic, CMYK, 4:4:0 / 4:1:1, 12-bit, multi-scan, ... or no JPEG at all), a file
whose EXIF orientation is not 1, a file whose entropy-coded data the device reports as damaged or as holding coefficients outside
the range in which every libjpeg computes the same bytes (``JPEG_S_RANGE``) and a file that ends without its EOI marker are
decoded by ``read_image_rgb`` itself -- same pixels, same exceptions.  Nothing here is a default anywhere:
``TrainBatches(decode="gpu")`` and ``generate_results_file(decode="gpu")`` opt in.

``encode_batch(images)`` is the way out: uint8 RGB or grey images on the GPU become baseline JPEG files, byte for byte the files
PIL writes for the same pixels, quality and subsampling (``csrc/jpeg_enc.hip``, nine launches per batch).
"""
import ctypes
import io
import os

import numpy as np
import torch

from . import _ffi
from ._staging import ALIGN, round_up

_INFO_BYTES = ctypes.sizeof(_ffi.JpegInfo)
_PROG_BYTES = ctypes.sizeof(_ffi.JpegProg)

ENTROPY = {"serial": 0, "parallel": 1}                    # enum YV3_JPEG_ENTROPY_* of include/yv3.h (no JPEG_* code of _ffi)

# for measurements and tests; "launches": the kernels the calls launched, as the library counts them where it launches them
# (yv3_jpeg_launch_count before and after the call); "prog_images": progressive images sent to the device
counters = {"calls": 0, "uploads": 0, "upload_bytes": 0, "status_reads": 0, "fallbacks": 0, "launches": 0, "prog_images": 0}


def read_bytes(source):
    """The bytes of a source: a path is read, ``bytes`` / ``bytearray`` / ``memoryview`` are taken as they are."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    with open(os.fspath(source), "rb") as f:
        return f.read()


def parse(data):
    """``yv3_jpeg_parse`` of ``data``: the ``_ffi.JpegInfo`` record (``reason`` 0 = a file the GPU decoder takes)."""
    info = _ffi.JpegInfo()
    _ffi.check(_ffi.lib().yv3_jpeg_parse(data, len(data), ctypes.byref(info)), "yv3_jpeg_parse")
    return info


def parse_ex(data, progressive=True):
    """``yv3_jpeg_parse_ex`` of ``data``: ``(info, prog)``.  ``prog`` is the ``_ffi.JpegProg`` record of an accepted progressive
    file (``info.reason`` then stays ``JPEG_PROGRESSIVE``) and None for every other file."""
    info, prog = _ffi.JpegInfo(), _ffi.JpegProg()
    _ffi.check(_ffi.lib().yv3_jpeg_parse_ex(data, len(data), _ffi.JPEGP_ACCEPT if progressive else 0, ctypes.byref(info),
                                            ctypes.byref(prog)), "yv3_jpeg_parse_ex")
    return info, (prog if prog.accepted else None)


def _pil(source, data):
    """`evaluate.read_image_rgb` of the source: of the path itself when there is one (same errors, same messages)."""
    from . import evaluate
    counters["fallbacks"] += 1
    if isinstance(source, (bytes, bytearray, memoryview)):
        return evaluate.read_image_rgb(io.BytesIO(data))
    return evaluate.read_image_rgb(source)


def _orientation(data):
    """The EXIF orientation, from PIL's header parse only (no pixel is decoded); 1 when PIL cannot tell."""
    from PIL import Image
    try:
        with Image.open(io.BytesIO(data)) as im:
            return int(im.getexif().get(0x0112, 1))
    except Exception:
        return 1


class Source:
    """One source ahead of the GPU: its bytes, its parsed record and, when it cannot go to the GPU decoder, either its pixels
    from `read_image_rgb` (``pixels``) or the exception that raised (``error``).  Built on any thread (`TrainBatches`' workers).
    ``progressive=True``: the file is parsed with the progressive flag, and ``prog`` is the record of an accepted progressive
    file (None for every other file)."""
    __slots__ = ("source", "data", "info", "prog", "pixels", "error", "shape", "unterminated")

    def __init__(self, source, progressive=False):
        self.source, self.pixels, self.error, self.prog = source, None, None, None
        self.data = read_bytes(source)
        if progressive:
            self.info, self.prog = parse_ex(self.data)
        else:
            self.info = parse(self.data)
        f = self.info
        gpu = (f.reason == 0 or self.prog is not None) and not (f.has_exif and _orientation(self.data) != 1)
        # a scan that runs to the end of the file has no EOI: PIL raises on such a file, whatever the device makes of its bits
        if self.prog is not None:
            last = self.prog.scans[self.prog.nscans - 1]
            self.unterminated = gpu and last.offset + last.length >= len(self.data)
        else:
            self.unterminated = gpu and f.scan_offset + f.scan_length >= len(self.data)
        if gpu:
            self.shape = (int(f.height), int(f.width))
        else:
            try:
                self.pixels = _pil(source, self.data)
                self.shape = tuple(self.pixels.shape[:2])
            except Exception as e:                          # raised where the image is used, as read_image_rgb would there
                self.error, self.shape = e, (0, 0)

    @property
    def on_gpu(self):
        return self.pixels is None and self.error is None

    @property
    def nbytes(self):
        return self.shape[0] * self.shape[1] * 3


class Decoded(list):
    """`decode_batch`'s result: a list of uint8 ``[H,W,3]`` GPU tensors.  ``fallback[i]``: image i took the PIL path;
    ``reasons[i]``: ``("parser", reason)``, ``("exif", None)``, ``("device", status)``, ``("truncated", None)`` or None;
    ``handed_over[i]``: the units of image i that ``entropy="parallel"`` handed to the serial routine on the device (0 for a file
    an encoder can write, and always with ``entropy="serial"`` or for an image that never reached the device)."""
    fallback = ()
    reasons = ()
    handed_over = ()


class Job:
    """A decode in flight on ``stream``, with an event recorded right after its own work.  `finish` waits for that event on the
    host, reads the statuses once, routes damaged files through PIL and makes the current stream wait for the event too.
    ``handed_over`` (one int per image, zeros until `finish`): see `Decoded`."""

    def __init__(self, items, views, reasons, status_host, event, stream, keep, parallel=False):
        self.items, self.views, self.reasons = items, views, reasons
        self.handed_over, self._parallel = [0] * len(items), parallel
        self._status_host, self._event, self._stream, self._keep = status_host, event, stream, keep
        self._finished = False

    def finish(self, errors="raise"):
        if not self._finished:
            self._finished = True
            self._event.synchronize()                        # this job's own kernels, not whatever the stream got after them
            redo = False
            if self._status_host is not None:
                counters["status_reads"] += 1
                status = self._status_host.numpy()           # [B] statuses, then (parallel) [B] hand-over counts: one read
                B = len(status) // 2 if self._parallel else len(status)
                k = 0
                for i, it in enumerate(self.items):
                    if not it.on_gpu:
                        continue
                    st = int(status[k])
                    if self._parallel:
                        self.handed_over[i] = int(status[B + k])
                    k += 1
                    if st == 0 and not it.unterminated:
                        continue
                    self.reasons[i] = ("device", st) if st else ("truncated", None)
                    try:
                        px = _pil(it.source, it.data)
                    except Exception as e:
                        it.error = e
                        continue
                    t = torch.from_numpy(px)
                    with torch.cuda.stream(self._stream):
                        if tuple(px.shape) == tuple(self.views[i].shape):
                            self.views[i].copy_(t)           # into the slot the device left unspecified
                        else:
                            self.views[i] = t.to(self.views[i].device)
                    redo = True
            if redo:                                         # the copies above: a fresh event after them
                self._event = torch.cuda.Event()
                self._event.record(self._stream)
        out = Decoded()
        for i, it in enumerate(self.items):
            if it.error is not None:
                if errors == "raise":
                    raise it.error
                out.append(it.error)
            else:
                out.append(self.views[i])
        out.fallback = [r is not None for r in self.reasons]
        out.reasons = list(self.reasons)
        out.handed_over = list(self.handed_over)
        cur = torch.cuda.current_stream(self._keep[0].device)
        if cur != self._stream:
            cur.wait_event(self._event)                      # the consumer waits for this job alone: a later job's decode on the
            for t in self._keep:                             # same stream (the next batch's) keeps running beside the consumer
                t.record_stream(cur)
        return out


def submit(sources, device=None, stream=None, dst=None, entropy="serial", progressive=False):
    """Enqueue the decode of ``sources`` (paths, ``bytes`` or prepared `Source` objects) on ``stream`` (default: the current one)
    and return the `Job`.  One device allocation holds, in this order, the upload -- records, offsets, the files' bytes and the
    pixels of the images PIL already decoded -- and the images the kernels write, each at a 256-aligned offset; it is filled by
    ONE host-to-device copy.  ``dst = (tensor, offsets)``: image i is decoded into the uint8 1-D ``tensor`` (`TrainBatches`'
    arena) at ``offsets[i]`` instead, for every i (None entries are not allowed: split the batch).  ``entropy="parallel"``: the
    self-synchronising entropy stage (``YV3_JPEG_ENTROPY_PARALLEL``) -- the same statuses and pixels; its hand-over counts lie
    behind the statuses and come back in the same read.  ``progressive=True``: sources are parsed with the progressive flag; an
    accepted progressive file goes to the device (``yv3_jpeg_decode_batch_prog``, one more launch), its record in the same
    upload and its status in the same read.  ``entropy`` affects the baseline images of the batch alone."""
    if entropy not in ENTROPY:
        raise ValueError("entropy must be 'serial' or 'parallel'")
    parallel = entropy == "parallel"
    if not torch.cuda.is_available():
        raise _ffi.Yv3Error("no GPU available: this package has no CPU path")
    dev = torch.device(device if device is not None else "cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    items = [s if isinstance(s, Source) else Source(s, progressive=progressive) for s in sources]
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    counters["calls"] += 1
    lib = _ffi.lib()
    gpu = [i for i, it in enumerate(items) if it.on_gpu]
    host_px = [i for i, it in enumerate(items) if it.pixels is not None]
    B = len(gpu)
    reasons = [None] * len(items)
    for i, it in enumerate(items):
        if not it.on_gpu:
            reasons[i] = ("parser", int(it.info.reason)) if it.info.reason and it.prog is None else ("exif", None)
    prog_of, progs = [], []                                  # per device image: the index of its progressive record, or -1
    for i in gpu:
        prog_of.append(len(progs) if items[i].prog is not None else -1)
        if items[i].prog is not None:
            progs.append(items[i].prog)
    P = len(progs)

    # layout of the allocation: infos | src offsets | dst offsets | status | [progressive records | their indices] | file bytes |
    # PIL pixels || decoded images
    o_info = 0
    o_soff = round_up(o_info + B * _INFO_BYTES)
    o_doff = round_up(o_soff + B * 8)
    o_stat = round_up(o_doff + B * 8)
    o_prog = round_up(o_stat + B * (8 if parallel else 4))  # parallel: [B] hand-over counts behind the statuses
    o_pof = round_up(o_prog + P * _PROG_BYTES)
    o_src = round_up(o_pof + (B * 4 if P else 0))           # (without a progressive image: the layout of a baseline batch)
    src_off, pos = [], o_src
    for i in gpu:
        src_off.append(pos - o_src)
        pos += len(items[i].data)                           # files are packed back to back: any byte offset will do
    src_bytes = max(pos - o_src, 1)
    pos = round_up(pos)
    px_off = {}
    for i in host_px:
        if dst is None:
            px_off[i] = pos
            pos = round_up(pos + items[i].nbytes)
    upload = pos
    own_off = {}
    if dst is None:
        for i in gpu:
            own_off[i] = pos
            pos = round_up(pos + items[i].nbytes)
    total = max(pos, 1)

    with torch.cuda.device(dev), torch.cuda.stream(stream):
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        staging = torch.empty(max(upload, 1), dtype=torch.uint8, pin_memory=True)
        host = staging.numpy()
        infos = (_ffi.JpegInfo * max(B, 1))()
        for k, i in enumerate(gpu):
            infos[k] = items[i].info
            d = items[i].data
            host[o_src + src_off[k]:o_src + src_off[k] + len(d)] = np.frombuffer(d, dtype=np.uint8)
        if B:
            host[o_info:o_info + B * _INFO_BYTES] = np.frombuffer(infos, dtype=np.uint8, count=B * _INFO_BYTES)
            host[o_soff:o_soff + B * 8].view(np.int64)[:] = src_off
        progs_host = prog_of_host = None                     # without a progressive image the calls below get null record pointers
        if P:
            prog_arr = (_ffi.JpegProg * P)(*progs)
            prog_of_arr = (ctypes.c_int * B)(*prog_of)
            progs_host, prog_of_host = ctypes.addressof(prog_arr), ctypes.addressof(prog_of_arr)
            host[o_prog:o_prog + P * _PROG_BYTES] = np.frombuffer(prog_arr, dtype=np.uint8, count=P * _PROG_BYTES)
            host[o_pof:o_pof + B * 4].view(np.int32)[:] = prog_of
        if dst is None:
            dst_t, dst_off = buf, [own_off[i] for i in gpu]
            views = [None] * len(items)
            for i, it in enumerate(items):
                if it.error is None:
                    off = own_off[i] if it.on_gpu else px_off[i]
                    views[i] = buf[off:off + it.nbytes].view(it.shape[0], it.shape[1], 3)
            for i in host_px:
                host[px_off[i]:px_off[i] + items[i].nbytes] = items[i].pixels.reshape(-1)
        else:
            dst_t, offsets = dst
            if dst_t.dtype != torch.uint8 or dst_t.dim() != 1 or not dst_t.is_contiguous() or dst_t.device != dev:
                raise _ffi.Yv3Error("dst must be a contiguous 1-D uint8 tensor on the decoding device")
            if len(offsets) != len(items) or any(o is None or o < 0 or o + it.nbytes > dst_t.numel() for o, it in zip(offsets, items)):
                raise _ffi.Yv3Error("dst offsets: one in-range offset per image")
            dst_off = [int(offsets[i]) for i in gpu]
            views = [None if it.error is not None else dst_t[int(o):int(o) + it.nbytes].view(it.shape[0], it.shape[1], 3)
                     for o, it in zip(offsets, items)]
        if B:
            host[o_doff:o_doff + B * 8].view(np.int64)[:] = dst_off
        if upload:
            buf[:upload].copy_(staging[:upload], non_blocking=True)
            counters["uploads"] += 1
            counters["upload_bytes"] += upload
        if dst is not None:
            for i in host_px:                               # PIL's pixels of a refused file go to the arena by a copy of their own
                views[i].copy_(torch.from_numpy(items[i].pixels), non_blocking=False)
        keep = [buf]
        status_host = None
        if B:
            ws_bytes = lib.yv3_jpeg_workspace_bytes_prog(ctypes.addressof(infos), prog_of_host, progs_host, P, B, ENTROPY[entropy])
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            base = buf.data_ptr()
            desc = _ffi.JpegBatchDesc(src=base + o_src, src_bytes=src_bytes, src_offsets=base + o_soff, infos=base + o_info,
                                      infos_host=ctypes.addressof(infos), dst=dst_t.data_ptr(), dst_bytes=dst_t.numel(),
                                      dst_offsets=base + o_doff, status=base + o_stat, B=B)
            handed = base + o_stat + B * 4 if parallel else None
            launched = lib.yv3_jpeg_launch_count()
            # (P == 0: the same four launches as yv3_jpeg_decode_batch_ex, by definition)
            pdesc = _ffi.JpegBatchDescProg(base=desc, progs=base + o_prog if P else None, progs_host=progs_host,
                                           prog_of=base + o_pof if P else None, prog_of_host=prog_of_host, P=P)
            _ffi.check(lib.yv3_jpeg_decode_batch_prog(ctypes.byref(pdesc), ENTROPY[entropy], handed, ws.data_ptr(), ws.numel(),
                                                      stream.cuda_stream), "yv3_jpeg_decode_batch_prog")
            counters["launches"] += lib.yv3_jpeg_launch_count() - launched
            counters["prog_images"] += P
            n_read = 2 * B if parallel else B
            status_host = torch.empty(n_read, dtype=torch.int32, pin_memory=True)
            status_host.copy_(buf[o_stat:o_stat + n_read * 4].view(torch.int32), non_blocking=True)
        event = torch.cuda.Event()                          # after this job's upload, kernels and status copy, and nothing else
        event.record(stream)
    return Job(items, views, reasons, status_host, event, stream, keep, parallel)


# ---- encode (csrc/jpeg_enc.hip) ------------------------------------------------------------------------
SUBSAMPLING = {"4:4:4": _ffi.JPEGE_444, "4:2:2": _ffi.JPEGE_422, "4:2:0": _ffi.JPEGE_420}
_ENC_BYTES = ctypes.sizeof(_ffi.JpegEncImage)


def encode_bound(width, height, ncomp, subsampling="4:2:0"):
    """``yv3_jpeg_encode_bound``: a length no file of this size and mode exceeds (raises beyond the encoder's size limit)."""
    n = _ffi.lib().yv3_jpeg_encode_bound(int(width), int(height), int(ncomp), SUBSAMPLING[subsampling])
    if n < 0:
        _ffi.check(int(n), "yv3_jpeg_encode_bound")
    return int(n)


def _encode_input(image, dev):
    """A uint8 GPU tensor ``[H,W,3]`` or ``[H,W]`` whose pixels are contiguous inside a row (rows may be pitched)."""
    if isinstance(image, torch.Tensor):
        t = image
    else:
        a = np.asarray(image)
        if a.dtype != np.uint8:
            raise TypeError("encode: images must be uint8, got %s" % a.dtype)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8:
        raise TypeError("encode: images must be uint8, got %s" % t.dtype)
    if not (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)) or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("encode: images must be [H, W, 3] or [H, W] with H, W >= 1, got %s" % (tuple(t.shape),))
    if not t.is_cuda:
        counters["uploads"] += 1
        counters["upload_bytes"] += t.numel()
        t = t.to(dev)
    elif t.device != dev:
        raise _ffi.Yv3Error("encode: an image lives on %s, the call runs on %s" % (t.device, dev))
    rows_ok = t.stride(1) == 1 if t.dim() == 2 else (t.stride(2) == 1 and t.stride(1) == 3)
    if not rows_ok or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * (1 if t.dim() == 2 else 3)):
        t = t.contiguous()
    return t


def encode_launch(tensors, qualities, subsamplings, out, offsets, capacities, ws=None, stream=None):
    """Enqueue ``yv3_jpeg_encode_batch`` for prepared GPU tensors (see `submit_encode`): image i's file goes to the uint8 1-D GPU
    tensor ``out`` at ``offsets[i]``, at most ``capacities[i]`` bytes.  ``ws``: a uint8 GPU tensor to use as the workspace when it
    is large enough (its contents do not matter), else one is allocated.  Returns ``(lengths, statuses, keep)``: two int32 GPU
    tensors ``[B]`` and the tensors that must stay alive until the stream has run the call.  Nothing here waits for the device."""
    lib = _ffi.lib()
    dev = out.device
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    B = len(tensors)
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise _ffi.Yv3Error("encode: out must be a contiguous 1-D uint8 tensor")
    if not (len(qualities) == len(subsamplings) == len(offsets) == len(capacities) == B) or B < 1:
        raise ValueError("encode: one quality, subsampling, offset and capacity per image")
    recs = (_ffi.JpegEncImage * B)()
    for i, t in enumerate(tensors):
        ncomp = 1 if t.dim() == 2 else 3
        if int(offsets[i]) < 0 or int(capacities[i]) < 0 or int(offsets[i]) + int(capacities[i]) > out.numel():
            raise _ffi.Yv3Error("encode: image %d's output range lies outside out" % i)
        recs[i] = _ffi.JpegEncImage(pixels=t.data_ptr(), pitch=t.stride(0) if t.shape[0] > 1 else t.shape[1] * ncomp,
                                    out=out.data_ptr() + int(offsets[i]), out_cap=int(capacities[i]), width=t.shape[1], height=t.shape[0],
                                    ncomp=ncomp, subsampling=int(subsamplings[i]), quality=int(qualities[i]))
    need = lib.yv3_jpeg_encode_workspace_bytes(recs, B)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        o_len = round_up(B * _ENC_BYTES)
        staging = torch.empty(o_len, dtype=torch.uint8, pin_memory=True)
        staging.numpy()[:B * _ENC_BYTES] = np.frombuffer(recs, dtype=np.uint8, count=B * _ENC_BYTES)
        meta = torch.empty(o_len + 8 * B, dtype=torch.uint8, device=dev)           # records | lengths [B] | statuses [B]
        meta[:o_len].copy_(staging, non_blocking=True)
        if ws is None or ws.numel() < need or ws.device != dev or ws.data_ptr() % ALIGN:
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        base = meta.data_ptr()
        desc = _ffi.JpegEncDesc(images=base, images_host=ctypes.addressof(recs), out_len=base + o_len, status=base + o_len + 4 * B, B=B)
        _ffi.check(lib.yv3_jpeg_encode_batch(ctypes.byref(desc), ws.data_ptr(), ws.numel(), stream.cuda_stream), "yv3_jpeg_encode_batch")
        both = meta[o_len:].view(torch.int32)
    return both[:B], both[B:], [meta, ws, staging, out] + list(tensors)


class EncodeJob:
    """An encode in flight: the files stay on the device until `finish`, which waits for this job's event, reads the lengths and
    statuses once, and copies the files' bytes -- packed back to back on the device first -- in one transfer."""

    def __init__(self, out, offsets, both_host, event, stream, keep):
        self._out, self._offsets, self._both_host, self._event, self._stream, self._keep = out, offsets, both_host, event, stream, keep
        self._result = None

    def finish(self):
        if self._result is None:
            self._event.synchronize()
            counters["status_reads"] += 1
            B = len(self._offsets)
            both = self._both_host.numpy()
            lengths, statuses = [int(v) for v in both[:B]], [int(v) for v in both[B:]]
            for i, st in enumerate(statuses):
                if st:
                    err = _ffi.Yv3Error("encode: image %d ended with device status %d" % (i, st))
                    err.code = st
                    raise err
            with torch.cuda.stream(self._stream):
                packed = torch.cat([self._out[o:o + n] for o, n in zip(self._offsets, lengths)]).cpu()
            data, pos, files = packed.numpy().tobytes(), 0, []
            for n in lengths:
                files.append(data[pos:pos + n])
                pos += n
            self._result, self._keep, self._out = files, None, None
        return list(self._result)


def submit_encode(images, quality=75, subsampling="4:2:0", device=None, stream=None):
    """Enqueue the baseline JPEG encode of ``images`` on ``stream`` (default: the current one) and return the `EncodeJob`.
    ``images``: uint8 ``[H,W,3]`` (RGB) or ``[H,W]`` (grey), GPU tensors or host arrays (which are uploaded); sizes and kinds may
    differ inside the batch; rows may be pitched (a row slice of a larger tensor is read in place).  ``quality`` 1..100 and
    ``subsampling`` (``"4:4:4"``, ``"4:2:2"``, ``"4:2:0"``; ignored for grey) are one value or one per image.  Every file is the
    one ``PIL.Image.save(..., "JPEG", quality=, subsampling=)`` writes for the same pixels, byte for byte."""
    images = list(images)
    B = len(images)
    qualities = list(quality) if isinstance(quality, (list, tuple)) else [quality] * max(B, 1)
    subs = list(subsampling) if isinstance(subsampling, (list, tuple)) else [subsampling] * max(B, 1)
    if len(qualities) != max(B, 1) or len(subs) != max(B, 1):
        raise ValueError("encode: one quality and one subsampling, or one per image")
    for q in qualities:
        if not isinstance(q, (int, np.integer)) or isinstance(q, bool) or not 1 <= q <= 100:
            raise ValueError("encode: quality must be an integer in 1..100, got %r" % (q,))
    for s in subs:
        if s not in SUBSAMPLING:
            raise ValueError("encode: subsampling must be one of %s, got %r" % (sorted(SUBSAMPLING), s))
    if not torch.cuda.is_available():
        raise _ffi.Yv3Error("no GPU available: this package has no CPU path")
    dev = torch.device(device if device is not None else "cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    if B == 0:
        job = EncodeJob(None, [], None, None, stream, None)
        job._result = []
        return job
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        tensors = [_encode_input(im, dev) for im in images]
        offsets, caps, pos = [], [], 0
        for t, s in zip(tensors, subs):
            cap = encode_bound(t.shape[1], t.shape[0], 1 if t.dim() == 2 else 3, s)
            offsets.append(pos)
            caps.append(cap)
            pos = round_up(pos + cap)
        out = torch.empty(pos, dtype=torch.uint8, device=dev)
        lengths, statuses, keep = encode_launch(tensors, qualities, [SUBSAMPLING[s] for s in subs], out, offsets, caps, stream=stream)
        both_host = torch.empty(2 * B, dtype=torch.int32, pin_memory=True)
        both_host[:B].copy_(lengths, non_blocking=True)
        both_host[B:].copy_(statuses, non_blocking=True)
        event = torch.cuda.Event()
        event.record(stream)
    return EncodeJob(out, offsets, both_host, event, stream, keep)


def encode_batch(images, quality=75, subsampling="4:2:0", device=None):
    """``list[bytes]``: the baseline JPEG file of every image, byte for byte the file PIL writes for the same pixels and settings
    (see `submit_encode`).  One read of the lengths and one transfer of the bytes per call."""
    return submit_encode(images, quality=quality, subsampling=subsampling, device=device).finish()


def decode_batch(sources, device=None, errors="raise", entropy="serial", progressive=False):
    """uint8 RGB ``[H,W,3]`` GPU tensors of ``sources`` (paths or ``bytes``), each what `evaluate.read_image_rgb` returns for it,
    as views into one allocation at 256-aligned offsets: a `Decoded` list whose ``fallback`` says which images took the PIL path.
    One upload (records + file bytes) and one status read per call.  ``errors="raise"`` (default): an image PIL cannot read
    raises what `read_image_rgb` raises; ``"keep"``: the exception takes the image's place in the list.  ``entropy``: ``"serial"``
    (default; one lane per restart segment or scan) or ``"parallel"`` (the self-synchronising stage): the same result either way.
    ``progressive=True``: progressive files whose script the parser accepts are decoded on the GPU too (the same pixels)."""
    if errors not in ("raise", "keep"):
        raise ValueError("errors must be 'raise' or 'keep'")
    return submit(sources, device=device, entropy=entropy, progressive=progressive).finish(errors)
