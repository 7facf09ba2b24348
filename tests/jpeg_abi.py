"""One call of the JPEG decoder through its C ABI, for the GPU tests: `decode` lays out a batch the hard way -- sources at odd
byte offsets, destinations of every alignment, fill values and guard bytes around the destinations, the workspace, the statuses
and the hand-over counts -- calls the entry asked for, and asserts that nothing but what the call owns was written."""
import ctypes
import types

import numpy as np
import torch

from yolo_v3_amd import _ffi, jpeg

DEV = "cuda:0"
GUARD = 512
FILL, WS_FILL, SRC_FILL, STATUS_FILL, HANDED_FILL = 0xA5, 0x3C, 0x5A, 777, 555
SERIAL, PARALLEL = jpeg.ENTROPY["serial"], jpeg.ENTROPY["parallel"]


def _device(array):
    return torch.from_numpy(np.frombuffer(array, np.uint8).copy()).to(DEV)


def decode(datas, entry="batch", entropy=SERIAL, order=None, handed_null=False, dev_infos=None, dev_progs=None, dst_cut=0):
    """One ``yv3_jpeg_decode_batch`` (``entry="batch"``), ``_ex`` (``"ex"``) or ``_prog`` (``"prog"``: files are parsed with the
    progressive flag, and a batch without a progressive file makes the call with P = 0 and null record pointers) over the files
    ``datas``, image k being file ``order[k]`` (default: each file once).  Every file is in the source buffer once, at an odd
    offset; the workspace has exactly the size the entry's own query gives.  ``dev_infos`` / ``dev_progs``: ctypes arrays whose
    bytes the DEVICE gets as records instead of the host's (records that lie).  ``dst_cut``: the call is told a destination buffer
    that ends this many bytes before the last image does.  ``handed_null``: no array for the hand-over counts.  Asserted here: the
    guards around every destination, the workspace, the statuses and the counts; the counts untouched unless the parallel stage
    got an array for them; the source bytes unchanged; for ``"ex"``, the workspace size equal to ``yv3_jpeg_workspace_bytes``'.
    Returns ``statuses``, ``handed`` (int arrays [B]), ``images`` ([H,W,3] arrays of the destination bytes: the fill value where
    the device wrote nothing), ``dst_off``, ``need`` and ``launches``."""
    order = list(range(len(datas))) if order is None else list(order)
    B = len(order)
    lib = _ffi.lib()
    infos, progs, prog_of = (_ffi.JpegInfo * B)(), [], []
    for k, j in enumerate(order):
        if entry == "prog":
            infos[k], rec = jpeg.parse_ex(datas[j])
        else:
            infos[k], rec = jpeg.parse(datas[j]), None
        assert infos[k].reason == 0 or rec is not None, (k, infos[k].reason)
        prog_of.append(len(progs) if rec is not None else -1)
        if rec is not None:
            progs.append(rec)
    P = len(progs)
    file_off, pos = [], 1
    for d in datas:
        file_off.append(pos)
        pos = (pos + len(d) + 3) | 1                                     # odd offsets
    src = np.full(pos + 7, SRC_FILL, np.uint8)
    for o, d in zip(file_off, datas):
        src[o:o + len(d)] = np.frombuffer(d, np.uint8)
    shapes = [(infos[k].height, infos[k].width, 3) for k in range(B)]
    sizes = [h * w * 3 for h, w, _ in shapes]
    dst_off, dpos = [], GUARD + 1
    for k in range(B):
        dst_off.append(dpos)
        dpos += sizes[k] + GUARD + (k % 3)                               # any alignment
    prog_host = (_ffi.JpegProg * P)(*progs) if P else None
    pof_host = (ctypes.c_int * B)(*prog_of) if P else None
    prog_host_p, pof_host_p = (ctypes.addressof(prog_host), ctypes.addressof(pof_host)) if P else (None, None)
    if entry == "batch":
        need = lib.yv3_jpeg_workspace_bytes(ctypes.addressof(infos), B)
    elif entry == "ex":
        need = lib.yv3_jpeg_workspace_bytes_ex(ctypes.addressof(infos), B, entropy)
        assert need == lib.yv3_jpeg_workspace_bytes(ctypes.addressof(infos), B)
    else:
        need = lib.yv3_jpeg_workspace_bytes_prog(ctypes.addressof(infos), pof_host_p, prog_host_p, P, B, entropy)
    assert need > 0
    dst = torch.full((dpos,), FILL, dtype=torch.uint8, device=DEV)
    ws = torch.full((need + 2 * GUARD,), WS_FILL, dtype=torch.uint8, device=DEV)
    d_src = torch.from_numpy(src).to(DEV)
    d_soff = torch.tensor([file_off[j] for j in order], dtype=torch.int64, device=DEV)
    d_doff = torch.tensor(dst_off, dtype=torch.int64, device=DEV)
    d_info = _device(dev_infos if dev_infos is not None else infos)
    status = torch.full((B + 2,), STATUS_FILL, dtype=torch.int32, device=DEV)
    handed = torch.full((B + 2,), HANDED_FILL, dtype=torch.int32, device=DEV)
    handed_p = None if handed_null or entry == "batch" else handed.data_ptr() + 4
    desc = _ffi.JpegBatchDesc(src=d_src.data_ptr(), src_bytes=d_src.numel(), src_offsets=d_soff.data_ptr(), infos=d_info.data_ptr(),
                              infos_host=ctypes.addressof(infos), dst=dst.data_ptr(),
                              dst_bytes=dst_off[-1] + sizes[-1] - dst_cut if dst_cut else dst.numel(), dst_offsets=d_doff.data_ptr(),
                              status=status.data_ptr() + 4, B=B)
    args = (ws.data_ptr() + GUARD, need, _ffi.stream_ptr())
    launched = lib.yv3_jpeg_launch_count()
    if entry == "batch":
        assert entropy == SERIAL
        _ffi.check(lib.yv3_jpeg_decode_batch(ctypes.byref(desc), *args), "yv3_jpeg_decode_batch")
    elif entry == "ex":
        _ffi.check(lib.yv3_jpeg_decode_batch_ex(ctypes.byref(desc), entropy, handed_p, *args), "yv3_jpeg_decode_batch_ex")
    else:
        if P:
            d_prog = _device(dev_progs if dev_progs is not None else prog_host)
            d_pof = torch.tensor(prog_of, dtype=torch.int32, device=DEV)
        pdesc = _ffi.JpegBatchDescProg(base=desc, progs=d_prog.data_ptr() if P else None, progs_host=prog_host_p,
                                       prog_of=d_pof.data_ptr() if P else None, prog_of_host=pof_host_p, P=P)
        _ffi.check(lib.yv3_jpeg_decode_batch_prog(ctypes.byref(pdesc), entropy, handed_p, *args), "yv3_jpeg_decode_batch_prog")
    launches = lib.yv3_jpeg_launch_count() - launched
    torch.cuda.synchronize()
    st, ho = status.cpu().numpy(), handed.cpu().numpy()
    assert st[0] == STATUS_FILL and st[-1] == STATUS_FILL and ho[0] == HANDED_FILL and ho[-1] == HANDED_FILL
    if entropy == SERIAL or handed_p is None:
        assert (ho == HANDED_FILL).all()                                 # not written by the serial stage, nor without an array
    got = dst.cpu().numpy()
    mask = np.ones(got.size, bool)
    images = []
    for k in range(B):
        mask[dst_off[k]:dst_off[k] + sizes[k]] = False
        images.append(got[dst_off[k]:dst_off[k] + sizes[k]].reshape(shapes[k]))
    assert (got[mask] == FILL).all()                                     # guard bytes around every destination
    wsn = ws.cpu().numpy()
    assert (wsn[:GUARD] == WS_FILL).all() and (wsn[GUARD + need:] == WS_FILL).all()      # and around the workspace
    assert (d_src.cpu().numpy() == src).all()
    return types.SimpleNamespace(statuses=st[1:-1], handed=ho[1:-1], images=images, dst_off=dst_off, need=need, launches=launches)
