"""The baseline JPEG encoder's host side, no GPU: the numpy restatement (tests/jpeg_enc_ref.py) against PIL's files, the shared
encoder code (csrc/jpeg_enc.h) walked in the kernels' order by a stand-alone program under ASan + UBSan, the header and bound
entry points, and the argument checks of the batch call.  Every comparison is equality with PIL's bytes."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_craft as jc  # noqa: E402
import jpeg_enc_ref as ref  # noqa: E402
from jpeg_checkers import build_checker, run_checker  # noqa: E402
from yolo_v3_amd import _ffi  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (24, 8), (8, 24), (33, 47), (40, 56), (64, 64), (96, 80)]      # (width, height)
QUALITIES = [1, 10, 50, 75, 90, 95, 100]
KINDS = ["noise", "binary", "smooth"]
SUB_CODE = {"grey": 0, "4:4:4": _ffi.JPEGE_444, "4:2:2": _ffi.JPEGE_422, "4:2:0": _ffi.JPEGE_420}


def grid():
    """The 924 cases: (width, height, mode, quality, kind, seed)."""
    n = 0
    for (w, h) in SIZES:
        for mode in ref.MODES:
            for q in QUALITIES:
                for kind in KINDS:
                    yield w, h, mode, q, kind, n
                    n += 1


_pil = {}


def pil_case(case):
    """(pixels, PIL's file) of a case, computed once."""
    if case not in _pil:
        w, h, mode, q, kind, seed = case
        a = ref.pixels(kind, w, h, mode == "grey", seed)
        _pil[case] = (a, ref.pil_file(a, q, mode))
    return _pil[case]


def header_of(data):
    """The bytes of a file up to and including its SOS segment."""
    pos = 2
    while data[pos + 1] != 0xDA:
        pos += 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0]
    return data[:pos + 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0]]


@pytest.mark.parametrize("mode", ref.MODES)
def test_reference_equals_pil_whole_files(mode):
    cases = [c for c in grid() if c[2] == mode]
    assert len(cases) == 231
    for case in cases:
        a, pil = pil_case(case)
        assert ref.encode(a, case[3], "4:4:4" if mode == "grey" else mode) == pil, case


def test_reference_tables_are_the_library_s():
    """The constants of csrc/jpeg_enc.h are the tables PIL writes (read from its files at run time)."""
    text = open(os.path.join(REPO, "yolo_v3_amd", "csrc", "jpeg_enc.h")).read()
    body = text[text.index("constexpr yv3_enc_spec YV3_ENC_SPEC"):text.index("// The encoder's view of the tables")]
    numbers = [int(v) for v in re.findall(r"\b\d+\b", body[body.index("{"):])]
    std, base = jc.standard_tables(), ref.base_tables()
    want = base[0] + base[1] + std[(0, 0)][0] + std[(0, 1)][0] + std[(0, 0)][1] + std[(0, 1)][1] + std[(1, 0)][0] + std[(1, 1)][0] \
        + std[(1, 0)][1] + std[(1, 1)][1] + jc.NATURAL_OF_ZIGZAG
    assert numbers == want


def test_header_entry_point_equals_pil_s_header():
    lib = _ffi.lib()
    seen = 0
    for case in grid():
        w, h, mode, q, kind, _ = case
        if kind != "noise":
            continue
        _, pil = pil_case(case)
        want = header_of(pil)
        ncomp = 1 if mode == "grey" else 3
        n = lib.yv3_jpeg_encode_header(w, h, ncomp, SUB_CODE[mode], q, None, 0)
        assert n == len(want), case
        buf = (ctypes.c_ubyte * n)()
        assert lib.yv3_jpeg_encode_header(w, h, ncomp, SUB_CODE[mode], q, buf, n) == n
        assert bytes(buf) == want, case
        short = (ctypes.c_ubyte * n)(*([0xAA] * n))                  # a smaller capacity: the same length, nothing past it
        assert lib.yv3_jpeg_encode_header(w, h, ncomp, SUB_CODE[mode], q, short, 100) == n
        assert bytes(short)[:100] == want[:100] and set(bytes(short)[100:]) == {0xAA}
        seen += 1
    assert seen == len(SIZES) * 4 * len(QUALITIES)
    assert lib.yv3_jpeg_encode_header(8, 8, 2, 0, 75, None, 0) == _ffi.EINVAL
    assert lib.yv3_jpeg_encode_header(8, 8, 3, 3, 75, None, 0) == _ffi.EINVAL
    assert lib.yv3_jpeg_encode_header(8, 8, 3, 0, 0, None, 0) == _ffi.EINVAL
    assert lib.yv3_jpeg_encode_header(8, 8, 3, 0, 101, None, 0) == _ffi.EINVAL
    assert lib.yv3_jpeg_encode_header(16385, 8, 3, 0, 75, None, 0) == _ffi.ELIMIT


def table_bound(w, h, mode):
    """Worst-case file bytes from the tables: per block the longest DC code of its table + 11 value bits and 63 times the longest
    AC code + 10 value bits, doubled for stuffing, plus PIL's header and EOI."""
    std = jc.standard_tables()
    longest = {key: max(i + 1 for i, c in enumerate(counts) if c) for key, (counts, _) in std.items()}
    hs, vs = (1, 1) if mode == "grey" else ref.SUBSAMPLING[mode]
    mcus = ((w + 8 * hs - 1) // (8 * hs)) * ((h + 8 * vs - 1) // (8 * vs))
    luma = longest[(0, 0)] + 11 + 63 * (longest[(1, 0)] + 10)
    chroma = longest[(0, 1)] + 11 + 63 * (longest[(1, 1)] + 10)
    bits = mcus * (luma if mode == "grey" else hs * vs * luma + 2 * chroma)
    return len(ref.header(w, h, 1 if mode == "grey" else 3, "4:4:4" if mode == "grey" else mode, 75)) + 2 * ((bits + 7) // 8) + 2


def test_bound_entry_point_covers_pil_and_the_tables():
    lib = _ffi.lib()
    for case in grid():
        w, h, mode, q, kind, _ = case
        _, pil = pil_case(case)
        bound = lib.yv3_jpeg_encode_bound(w, h, 1 if mode == "grey" else 3, SUB_CODE[mode])
        assert bound >= len(pil), case
        assert bound >= table_bound(w, h, mode), case
    assert lib.yv3_jpeg_encode_bound(4096, 4096, 3, _ffi.JPEGE_444) >= table_bound(4096, 4096, "4:4:4")
    assert lib.yv3_jpeg_encode_bound(16384, 16384, 3, _ffi.JPEGE_444) == _ffi.ELIMIT
    assert lib.yv3_jpeg_encode_bound(0, 8, 3, 0) == _ffi.EINVAL


def test_batch_call_checks_its_arguments_before_launching():
    """Dummy device pointers: every answer comes from the host checks, so nothing is launched (and no GPU is needed)."""
    lib = _ffi.lib()

    def image(**kw):
        f = dict(pixels=4096, pitch=24, out=8192, out_cap=4096, width=8, height=8, ncomp=3, subsampling=2, quality=75)
        f.update(kw)
        return _ffi.JpegEncImage(**f)

    def call(im, ws=256, ws_bytes=1 << 30, B=1, **kw):
        arr = (_ffi.JpegEncImage * 1)(im)
        f = dict(images=4096, images_host=ctypes.addressof(arr), out_len=4096, status=4096, B=B)
        f.update(kw)
        return lib.yv3_jpeg_encode_batch(ctypes.byref(_ffi.JpegEncDesc(**f)), ws, ws_bytes, None)

    good = (_ffi.JpegEncImage * 1)(image())
    need = lib.yv3_jpeg_encode_workspace_bytes(good, 1)
    assert need > 0 and need % 256 == 0
    assert call(image(), ws_bytes=need - 1) == _ffi.EWORKSPACE
    assert call(image(), ws=260) == _ffi.EINVAL
    assert call(image(), images=None) == _ffi.EINVAL
    assert call(image(), B=0) == _ffi.EINVAL
    for bad in (dict(width=0), dict(ncomp=2), dict(subsampling=3), dict(quality=0), dict(quality=101), dict(pitch=23), dict(pixels=None),
                dict(out=None), dict(out_cap=-1)):
        assert call(image(**bad)) == _ffi.EINVAL, bad
    assert call(image(width=16385, pitch=3 * 16385)) == _ffi.ELIMIT
    assert call(image(width=16384, height=16384, pitch=3 * 16384, subsampling=0)) == _ffi.ELIMIT      # 12.6 million blocks
    big = (_ffi.JpegEncImage * 1)(image(width=4096, height=4096, pitch=3 * 4096, subsampling=0))
    assert lib.yv3_jpeg_encode_workspace_bytes(big, 1) > 0                                            # the documented size is inside the limit
    assert lib.yv3_jpeg_encode_workspace_bytes(good, 0) == 0


@pytest.mark.parametrize("ctype,cname", [(_ffi.JpegEncImage, "yv3_jpeg_enc_image"), (_ffi.JpegEncDesc, "yv3_jpeg_enc_desc")])
def test_struct_layouts_match_the_c_header(tmp_path, ctype, cname):
    fields = [f for f, _ in ctype._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv3.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % cname
                   + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields]


def test_shared_encoder_code_in_the_kernels_order_equals_pil(tmp_path):
    """csrc/jpeg_enc.h on the CPU (tests/jpeg_enc_host_check.cpp, ASan + UBSan): coefficients, sizes, prefix sum, blocks written at
    their own bit offsets in reverse order, stuffing -- the whole grid in one run of the program."""
    checker = build_checker("jpeg_enc_host_check.cpp", tmp_path / "jpeg_enc_host_check")
    cases = list(grid())
    with open(tmp_path / "in.bin", "wb") as f:
        for case in cases:
            w, h, mode, q, kind, _ = case
            a, _ = pil_case(case)
            f.write(struct.pack("<5i", w, h, 1 if mode == "grey" else 3, SUB_CODE[mode], q) + a.tobytes())
    assert run_checker(checker, tmp_path / "in.bin", tmp_path / "out.bin").strip() == "encoded %d" % len(cases)
    out, pos = (tmp_path / "out.bin").read_bytes(), 0
    for case in cases:
        n = struct.unpack_from("<i", out, pos)[0]
        assert out[pos + 4:pos + 4 + n] == pil_case(case)[1], case
        pos += 4 + n
    assert pos == len(out)
