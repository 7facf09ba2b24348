"""The host half of the JPEG decoder (csrc/jpeg_parse.cpp, csrc/jpeg_entropy.h, csrc/jpeg_pixel.h), without a GPU: the parser's
fields against PIL, every refusal with its reason, the ctypes mirrors against the header, the argument checks that answer before
any launch, and a stand-alone sanitizer build (its own ``main``, never loaded into Python) that runs the parser, the entropy
routine and the pixel arithmetic over valid, truncated, corrupted and random inputs."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image, JpegImagePlugin

from tests.jpeg_checkers import build_checker, run_checker          # noqa: F401 (run_checker: tests.test_jpeg_craft_host's too)
from yolo_v3_amd import _ffi, jpeg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHOTO = os.path.join(REPO, "tests", "golden", "x_wing_0001.jpg")


def picture(w, h, mode="RGB", kind="noise", seed=0):
    c = 1 if mode == "L" else 3
    if kind == "flat":
        a = np.full((h, w, c), 77, np.uint8)
    elif kind == "gradient":
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)][:c], -1).astype(np.uint8)
    else:
        a = np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(np.uint8)
    return Image.fromarray(a[..., 0] if c == 1 else a, mode)


def encode(im, **kw):
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def patch_sof(data, offset, value):
    """``data`` with byte ``offset`` of its SOF0 payload replaced (0: precision, 7: the first component's sampling factors)."""
    i = data.index(b"\xff\xc0")
    out = bytearray(data)
    out[i + 4 + offset] = value
    return bytes(out)


@pytest.mark.parametrize("mode,subsampling,size,restart", [
    ("RGB", 0, (33, 19), None), ("RGB", 1, (17, 13), 2), ("RGB", 2, (64, 48), 2), ("RGB", 2, (1, 1), None), ("L", None, (7, 9), 3),
    ("RGB", 2, (40, 1), None), ("RGB", 1, (1, 40), None)])
def test_parser_fields_match_pil(mode, subsampling, size, restart):
    kw = {"quality": 75}
    if subsampling is not None:
        kw["subsampling"] = subsampling
    if restart:
        kw["restart_marker_blocks"] = restart
    data = encode(picture(size[0], size[1], mode), **kw)
    f = jpeg.parse(data)
    with Image.open(io.BytesIO(data)) as im:
        assert f.reason == _ffi.JPEG_OK
        assert (f.width, f.height) == im.size
        assert f.ncomp == (1 if mode == "L" else 3)
        if mode == "RGB":
            assert JpegImagePlugin.get_sampling(im) == subsampling
            assert (f.h[0], f.v[0]) == {0: (1, 1), 1: (2, 1), 2: (2, 2)}[subsampling]
            assert [(f.h[c], f.v[c]) for c in (1, 2)] == [(1, 1), (1, 1)]
            assert [f.tq[c] for c in range(3)] == [layer[3] for layer in im.layer]
        # (im.quantization is in natural order in current Pillow and was in the file's zigzag order in old ones)
        pil_q = {k: [int(v) for v in np.asarray(q)] for k, q in im.quantization.items()}
        assert pil_q in ({k: [f.quant[k][n] for n in range(64)] for k in range(4) if f.quant_defined[k]},
                         {k: [f.quant[k][n] for n in NATURAL_OF_ZIGZAG] for k in range(4) if f.quant_defined[k]})
    assert f.restart_interval == (restart or 0)
    assert f.has_exif == 0
    assert 0 < f.scan_offset and f.scan_offset + f.scan_length == len(data) - 2 and data[-2:] == b"\xff\xd9"


# natural index of zigzag position k
NATURAL_OF_ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                     49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def test_restart_rows_and_exif_flag():
    im = picture(64, 48)
    f = jpeg.parse(encode(im, subsampling=2, restart_marker_rows=1))
    assert f.reason == 0 and f.restart_interval == 4                      # 64 / 16 MCUs per row
    exif = Image.Exif()
    exif[0x0112] = 6
    data = encode(im, exif=exif)
    f = jpeg.parse(data)
    assert f.reason == 0 and f.has_exif == 1
    src = jpeg.Source(data)                                               # orientation 6: PIL's path, the rotated image
    assert not src.on_gpu and src.shape == (64, 48)
    exif[0x0112] = 1
    assert jpeg.Source(encode(im, exif=exif)).on_gpu


def test_refusals_carry_their_reason():
    rgb = picture(33, 19)
    base = encode(rgb, subsampling=0)
    adobe = base[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + base[2:]
    cases = {
        "progressive": (encode(rgb, progressive=True), _ffi.JPEG_PROGRESSIVE),
        "cmyk": (encode(picture(33, 19).convert("CMYK")), _ffi.JPEG_COMPONENTS),
        "4:1:1": (patch_sof(base, 7, 0x41), _ffi.JPEG_SAMPLING),
        "4:4:0": (patch_sof(base, 7, 0x12), _ffi.JPEG_SAMPLING),
        "adobe": (adobe, _ffi.JPEG_COLORSPACE),
        "12-bit": (patch_sof(base, 0, 12), _ffi.JPEG_PRECISION),
        "png": (b"\x89PNG\r\n\x1a\n" + bytes(64), _ffi.JPEG_NOT_JPEG),
        "empty": (b"", _ffi.JPEG_NOT_JPEG),
        "header only": (base[:200], _ffi.JPEG_MALFORMED),
        "two scans": (base[:-2] + base[base.index(b"\xff\xda"):], _ffi.JPEG_MULTISCAN),
        "too wide": (patch_sof(patch_sof(base, 3, 0x40), 4, 0x01), _ffi.JPEG_SIZE),        # width 16385
        "no huffman tables": (base[:base.index(b"\xff\xc4")] + base[base.index(b"\xff\xda"):], _ffi.JPEG_TABLES),
    }
    for name, (data, reason) in cases.items():
        assert jpeg.parse(data).reason == reason, name
    # PIL's own subsampling="4:1:1" is an alias of 4:2:0 (JpegImagePlugin, "for compatibility"): such a file is a 4:2:0 file,
    # which the parser takes like any other -- the refusal above is of a real 4:1:1 frame header
    pil_411 = encode(rgb, subsampling="4:1:1")
    with Image.open(io.BytesIO(pil_411)) as im:
        assert JpegImagePlugin.get_sampling(im) == 2
    assert jpeg.parse(pil_411).reason == 0
    # a truncated scan is the device's to find: the parser hands it over with the bytes there are
    cut = jpeg.parse(base[:-40])
    assert cut.reason == 0 and cut.scan_offset + cut.scan_length == len(base) - 40
    assert jpeg.Source(base[:-40]).unterminated and not jpeg.Source(base).unterminated


@pytest.mark.parametrize("ctype,cname", [(_ffi.JpegInfo, "yv3_jpeg_info"), (_ffi.JpegBatchDesc, "yv3_jpeg_batch_desc")])
def test_struct_layouts_match_the_c_header(tmp_path, ctype, cname):
    """The structs as ctypes sees them == as a C compiler sees include/yv3.h (size and every field offset)."""
    fields = [f for f, _ in ctype._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv3.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % cname
                   + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields]


def test_ffi_names_the_header_codes():
    header = open(os.path.join(REPO, "include", "yv3.h")).read()
    import re
    codes = {n: int(v) for n, v in re.findall(r"#define YV3_(JPEG_[A-Z_]+)\s+(\d+)", header)}
    assert len(codes) == 22
    assert codes == {n: v for n, v in vars(_ffi).items() if n.startswith("JPEG_")}


def test_decode_batch_checks_its_arguments_before_launching():
    """Dummy device pointers: every answer here comes from the host checks, so nothing is launched (and no GPU is needed)."""
    lib = _ffi.lib()
    infos = (_ffi.JpegInfo * 2)()
    infos[0] = jpeg.parse(encode(picture(33, 19), subsampling=2))
    infos[1] = jpeg.parse(encode(picture(7, 9, "L")))
    host = ctypes.addressof(infos)
    need = lib.yv3_jpeg_workspace_bytes(host, 2)
    # 2 slot records, then per image coefficients (128 B / block), planes (64 B / block) and restart offsets, 256-aligned
    assert need == 256 + (36 * 128 + 36 * 64 + 256) + (2 * 128 + 256 + 256)     # 33x19 4:2:0: 24 + 6 + 6 blocks; 7x9 grey: 2
    assert lib.yv3_jpeg_workspace_bytes(None, 2) == 0 and lib.yv3_jpeg_workspace_bytes(host, 0) == 0

    def desc(**kw):
        d = _ffi.JpegBatchDesc(src=4096, src_bytes=1000, src_offsets=4096, infos=4096, infos_host=host, dst=4096, dst_bytes=5000,
                               dst_offsets=4096, status=4096, B=2)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert lib.yv3_jpeg_decode_batch(desc(), 4096, need - 1, None) == _ffi.EWORKSPACE
    assert lib.yv3_jpeg_decode_batch(None, 4096, need - 1, None) == _ffi.EINVAL
    assert lib.yv3_jpeg_decode_batch(desc(B=0), None, need - 1, None) == _ffi.EINVAL
    # (every call carries a second defect -- here a workspace one byte short -- so that no single lost check could launch anything)
    for field in ("src", "src_offsets", "infos", "infos_host", "dst", "dst_offsets", "status"):
        assert lib.yv3_jpeg_decode_batch(desc(**{field: None}), 4096, need - 1, None) == _ffi.EINVAL, field
    assert lib.yv3_jpeg_decode_batch(desc(), 4096 + 8, need - 1, None) == _ffi.EINVAL          # ws must be 256-aligned
    for field, value in (("B", 0), ("B", 65536), ("src_bytes", 0), ("dst_bytes", -1)):
        assert lib.yv3_jpeg_decode_batch(desc(**{field: value}), 4096, 1 << 40, None) == _ffi.EINVAL, field
    refused = (_ffi.JpegInfo * 2)()
    refused[0], refused[1] = infos[0], jpeg.parse(encode(picture(33, 19), progressive=True))
    assert lib.yv3_jpeg_decode_batch(desc(infos_host=ctypes.addressof(refused)), 4096, 1 << 40, None) == _ffi.ESHAPE
    assert lib.yv3_jpeg_parse(None, 0, ctypes.byref(infos[0])) == _ffi.EINVAL


# ---- the stand-alone sanitizer program -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker("jpeg_host_check.cpp", tmp_path_factory.mktemp("jpeg_host") / "jpeg_host_check")


HOST_CASES = [("RGB", 2, (33, 19), 75, False, None), ("RGB", 1, (17, 13), 30, True, 2), ("RGB", 0, (7, 9), 100, False, None),
              ("L", None, (40, 1), 95, True, 2), ("RGB", 2, (2, 5), 75, False, None), ("RGB", 1, (3, 3), 75, False, None),
              ("RGB", 2, (64, 48), 95, True, "rows")]


@pytest.mark.parametrize("mode,subsampling,size,quality,optimize,restart", HOST_CASES)
def test_host_restatement_equals_pil(checker, tmp_path, mode, subsampling, size, quality, optimize, restart):
    """The code the kernels run (same headers), serially on the host under ASan + UBSan: bit for bit PIL's pixels."""
    kw = {"quality": quality, "optimize": optimize}
    if subsampling is not None:
        kw["subsampling"] = subsampling
    if restart == "rows":
        kw["restart_marker_rows"] = 1
    elif restart:
        kw["restart_marker_blocks"] = restart
    data = encode(picture(size[0], size[1], mode), **kw)
    (tmp_path / "in.jpg").write_bytes(data)
    assert run_checker(checker, "decode", tmp_path / "in.jpg", tmp_path / "out.rgb").strip() == "reason 0 status 0"
    head, _, px = (tmp_path / "out.rgb").read_bytes().partition(b"\n")
    w, h = (int(v) for v in head.split())
    ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert (h, w, 3) == ref.shape and np.array_equal(np.frombuffer(px, np.uint8).reshape(h, w, 3), ref)


def test_host_restatement_equals_pil_on_the_photograph(checker, tmp_path):
    assert os.path.getsize(PHOTO) < 50 * 1024
    assert run_checker(checker, "decode", PHOTO, tmp_path / "out.rgb").strip() == "reason 0 status 0"
    head, _, px = (tmp_path / "out.rgb").read_bytes().partition(b"\n")
    with Image.open(PHOTO) as im:
        assert im.size == (1280, 546) and JpegImagePlugin.get_sampling(im) == 2
        ref = np.asarray(im.convert("RGB"))
    assert head == b"1280 546" and np.array_equal(np.frombuffer(px, np.uint8).reshape(546, 1280, 3), ref)


@pytest.mark.parametrize("kw", [dict(subsampling=2, restart_marker_blocks=2), dict(subsampling=1, optimize=True), dict(subsampling=0)])
def test_damaged_inputs_end_in_a_status_under_the_sanitizers(checker, tmp_path, kw):
    """Every prefix truncation, 2000 seeded single-byte corruptions, 500 random tails after the valid header and 300 damaged
    header bytes of a small file, each on an exact-size heap copy: a clean exit, and a (reason, status) for every input."""
    data = encode(picture(33, 19, seed=3), quality=75, **kw)
    (tmp_path / "in.jpg").write_bytes(data)
    out = run_checker(checker, "fuzz", tmp_path / "in.jpg", 7)
    lines = out.strip().splitlines()
    assert lines[0] == "inputs %d" % (len(data) + 2800)
    seen = {(int(l.split()[1]), int(l.split()[3])): int(l.split()[5]) for l in lines[1:]}
    assert sum(seen.values()) == len(data) + 2800
    assert all(0 <= r <= 11 and 0 <= s <= 9 and not (r and s) for r, s in seen)
    # every class of outcome is met: refused headers, overruns of truncated scans, bad codes / runs in corrupted ones
    assert any(r for r, _ in seen) and (0, _ffi.JPEG_S_OVERRUN) in seen
    assert {s for _, s in seen} & {_ffi.JPEG_S_CODE, _ffi.JPEG_S_COEF}
