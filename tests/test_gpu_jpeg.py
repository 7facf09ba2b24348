"""The GPU JPEG decoder (csrc/jpeg.hip through yolo_v3_amd.jpeg) against PIL's decode of the same bytes in the same process,
bit for bit: tiny PIL-written files over every mode, subsampling, size, quality, Huffman-table and restart setting at once,
one real photograph, and the error paths (damaged and refused files come back through PIL; the host checks answer first)."""
import ctypes
import io
import itertools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_abi
from tests.test_jpeg_host import PHOTO, encode, picture
from yolo_v3_amd import _ffi, evaluate, jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 13), (33, 19), (40, 1), (1, 40), (64, 48)]
# widths at which libjpeg replaces fancy upsampling by replication (jinit_upsampler: chroma planes of one or two columns)
NARROW = [(2, 5), (3, 3), (4, 6), (5, 4), (6, 3)]


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.fixture(scope="module")
def files():
    """Every combination of the settings below, as (name, bytes), and PIL's pixels of each (computed once, never modified)."""
    out = []
    combos = itertools.product(SIZES + NARROW, ("flat", "gradient", "noise"), ("L", 0, 1, 2), (30, 75, 95, 100), (False, True),
                               (None, "blocks", "rows"))
    for n, ((w, h), kind, sub, q, opt, rst) in enumerate(combos):
        if (w, h) in NARROW and (q != 75 or kind == "flat" or sub == "L"):
            continue
        kw = {"quality": q, "optimize": opt}
        if sub != "L":
            kw["subsampling"] = sub
        if rst == "blocks":
            kw["restart_marker_blocks"] = 2
        elif rst == "rows":
            kw["restart_marker_rows"] = 1
        data = encode(picture(w, h, "L" if sub == "L" else "RGB", kind, seed=n), **kw)
        out.append(("%dx%d %s %s q%d opt%d %s" % (w, h, kind, sub, q, opt, rst), data))
    refs = [pil_rgb(d) for _, d in out]
    for r in refs:
        r.setflags(write=False)
    return out, refs


def test_every_setting_in_one_mixed_batch_through_the_c_abi(files):
    """One yv3_jpeg_decode_batch over all files: sources packed at odd byte offsets, one source used twice, every destination
    between guard bytes that must stay as they were, every status 0, every pixel PIL's."""
    cases, refs = files
    assert len(cases) == 9 * 3 * 4 * 4 * 2 * 3 + 5 * 2 * 3 * 2 * 3
    order = list(range(len(cases))) + [5]                               # file 5 is decoded twice, from the same bytes
    r = jpeg_abi.decode([d for _, d in cases], order=order)
    assert any(o % 4 for o in r.dst_off) and any(o % 4 == 0 for o in r.dst_off)
    bad = [(cases[j][0], int(s)) for j, s in zip(order, r.statuses) if s]
    assert not bad, bad[:10]
    wrong = [cases[j][0] for j, px in zip(order, r.images) if not np.array_equal(px, refs[j])]
    assert not wrong, (len(wrong), wrong[:10])


def test_decode_batch_one_upload_one_status_read(files):
    cases, refs = files
    pick = list(range(0, len(cases), 37))
    before = dict(jpeg.counters)
    out = jpeg.decode_batch([cases[j][1] for j in pick], device=DEV)
    assert {k: jpeg.counters[k] - before[k] for k in ("calls", "uploads", "status_reads", "fallbacks")} == \
        {"calls": 1, "uploads": 1, "status_reads": 1, "fallbacks": 0}
    assert isinstance(out, list) and out.fallback == [False] * len(pick) and out.reasons == [None] * len(pick)
    storage = {t.untyped_storage().data_ptr() for t in out}
    assert len(storage) == 1
    for t, j in zip(out, pick):
        assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and (t.data_ptr() - min(storage)) % 256 == 0
        assert np.array_equal(t.cpu().numpy(), refs[j]), cases[j][0]


def test_the_photograph_from_a_path_and_from_bytes():
    data = open(PHOTO, "rb").read()
    ref = pil_rgb(data)
    assert ref.shape == (546, 1280, 3)
    out = jpeg.decode_batch([PHOTO, data, PHOTO], device=DEV)
    assert out.fallback == [False, False, False]
    for t in out:
        assert np.array_equal(t.cpu().numpy(), ref)
    assert np.array_equal(out[0].cpu().numpy(), evaluate.read_image_rgb(PHOTO))


def damaged_files():
    good = encode(picture(64, 48, seed=11), quality=90, subsampling=2)
    info = jpeg.parse(good)
    mid = int(info.scan_offset + info.scan_length // 2)
    truncated = good[:mid]
    corrupted = good[:mid] + b"\xff\x00" * 4 + good[mid + 8:]            # 32 one-bits: no Huffman code is all ones
    return good, truncated, corrupted


def test_damaged_and_refused_files_come_back_through_pil():
    good, truncated, corrupted = damaged_files()
    other = encode(picture(33, 19, seed=12), quality=75, subsampling=1, restart_marker_blocks=2)
    progressive = encode(picture(17, 13, seed=13), progressive=True)
    exif = Image.Exif()
    exif[0x0112] = 6
    rotated = encode(picture(40, 24, seed=14), exif=exif)
    lost_marker = other.replace(b"\xff\xd1", b"\x12\x34", 1)              # a restart marker overwritten: count and order are off
    assert lost_marker != other
    batch = [good, truncated, other, corrupted, progressive, rotated, lost_marker, good]
    out = jpeg.decode_batch(batch, device=DEV, errors="keep")
    assert out.fallback == [False, True, False, True, True, True, True, False]
    assert out.reasons[1][0] == "device" and out.reasons[1][1] != 0
    assert out.reasons[3] == ("device", _ffi.JPEG_S_CODE)
    assert out.reasons[4] == ("parser", _ffi.JPEG_PROGRESSIVE) and out.reasons[5] == ("exif", None)
    assert out.reasons[6] == ("device", _ffi.JPEG_S_MARKER)
    for i, data in enumerate(batch):
        try:
            ref = evaluate.read_image_rgb(io.BytesIO(data))
        except Exception as e:                                           # a fallback behaves as read_image_rgb does, errors included
            assert type(out[i]) is type(e) and str(out[i]) == str(e), i
            assert i == 1
            continue
        assert np.array_equal(out[i].cpu().numpy(), ref), i
    assert out[5].shape == (40, 24, 3)
    with pytest.raises(OSError, match="truncated"):
        jpeg.decode_batch(batch, device=DEV)
    # a file cut right after its last entropy-coded byte decodes on the device, but PIL refuses a file without EOI: so do we
    out = jpeg.decode_batch([good, good[:-2]], device=DEV, errors="keep")
    assert out.reasons == [None, ("truncated", None)] and isinstance(out[1], OSError)
    assert np.array_equal(out[0].cpu().numpy(), pil_rgb(good))
    # a path that does not exist, and a file that is no image: read_image_rgb's own exceptions
    with pytest.raises(FileNotFoundError):
        jpeg.decode_batch([os.path.join(os.path.dirname(PHOTO), "missing.jpg")], device=DEV)
    with pytest.raises(Exception) as err:
        jpeg.decode_batch([b"not an image"], device=DEV)
    with pytest.raises(type(err.value)):
        evaluate.read_image_rgb(io.BytesIO(b"not an image"))


def lying_records(good):
    """Four records of the file ``good`` for the DEVICE: 1 lies about its scan's length, 2 about its width."""
    infos = (_ffi.JpegInfo * 4)()
    for k in range(4):
        infos[k] = jpeg.parse(good)
    infos[1].scan_length = 1 << 40                                       # the device copies lie; the host copies size the workspace
    infos[2].width = 20000
    return infos


def test_device_checks_keep_a_lying_record_inside_its_buffers():
    """Records whose fields do not fit the buffers they come with, and a destination buffer that ends one byte before the last
    image does: status BOUNDS / INFO per image, the neighbour untouched by it."""
    good, _, _ = damaged_files()
    r = jpeg_abi.decode([good], order=[0, 0, 0, 0], dev_infos=lying_records(good), dst_cut=1)
    assert r.statuses.tolist() == [0, _ffi.JPEG_S_BOUNDS, _ffi.JPEG_S_INFO, _ffi.JPEG_S_BOUNDS]
    assert np.array_equal(r.images[0], pil_rgb(good)) and all((px == jpeg_abi.FILL).all() for px in r.images[1:])


def test_host_checks_answer_before_any_launch():
    good, _, _ = damaged_files()
    lib = _ffi.lib()
    infos = (_ffi.JpegInfo * 1)()
    infos[0] = jpeg.parse(good)
    need = lib.yv3_jpeg_workspace_bytes(ctypes.addressof(infos), 1)
    d_src = torch.from_numpy(np.frombuffer(good, np.uint8).copy()).to(DEV)
    zero = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_info = torch.from_numpy(np.frombuffer(infos, np.uint8).copy()).to(DEV)
    dst = torch.full((64 * 48 * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.full((need,), 0x3C, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), 777, dtype=torch.int32, device=DEV)

    def call(ws_bytes=need, **kw):
        d = _ffi.JpegBatchDesc(src=d_src.data_ptr(), src_bytes=d_src.numel(), src_offsets=zero.data_ptr(), infos=d_info.data_ptr(),
                               infos_host=ctypes.addressof(infos), dst=dst.data_ptr(), dst_bytes=dst.numel(), dst_offsets=zero.data_ptr(),
                               status=status.data_ptr(), B=1)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.yv3_jpeg_decode_batch(ctypes.byref(d), ws.data_ptr(), ws_bytes, _ffi.stream_ptr())
    assert call(ws_bytes=need - 1) == _ffi.EWORKSPACE
    assert call(B=0) == _ffi.EINVAL and call(src=None) == _ffi.EINVAL and call(status=None) == _ffi.EINVAL and call(dst_bytes=0) == _ffi.EINVAL
    torch.cuda.synchronize()
    assert status.item() == 777 and (dst == 0xA5).all() and (ws == 0x3C).all()           # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert status.item() == 0 and np.array_equal(dst.cpu().numpy().reshape(48, 64, 3), pil_rgb(good))
