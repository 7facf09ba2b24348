"""The host restatement of the JPEG decoder (tests/jpeg_host_check.cpp: the headers the kernels run, under ASan + UBSan, its own
``main``, never loaded into Python) on files PIL's encoder does not write (tests/jpeg_craft.py), and on damaged files with a
PIXEL check: whatever comes back with ``reason 0 status 0`` holds exactly PIL's pixels.

  family A, B   every feature of the accepted set and every extreme an 8-bit encoder reaches: status 0 and PIL's pixels.  This is
                also the cap on the IDCT range guard (YV3_JPEG_S_RANGE): nothing an encoder can produce may be refused.
  family C      free coefficients: a non-zero status or PIL's pixels, and YV3_JPEG_S_RANGE where the issue is known to bite
  corruptions   300 seeded single-byte corruptions of the scan of three small files: a non-zero status or PIL's pixels

One subprocess per input."""
import io
import warnings

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_craft
from tests.test_jpeg_host import checker, run_checker                 # noqa: F401 (checker is a fixture)
from yolo_v3_amd import _ffi, evaluate, jpeg


def pil_rgb(data):
    """`evaluate.read_image_rgb` of the bytes, with every Python warning an error."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return evaluate.read_image_rgb(io.BytesIO(data))


def host_decode(checker, tmp_path, data):
    """(reason, status, pixels [H,W,3] or None) from the stand-alone program's ``decode`` mode."""
    src, dst = tmp_path / "in.jpg", tmp_path / "out.rgb"
    src.write_bytes(data)
    words = run_checker(checker, "decode", src, dst).split()
    assert words[0] == "reason" and words[2] == "status" and len(words) == 4
    reason, status = int(words[1]), int(words[3])
    if reason or status:
        return reason, status, None
    head, _, px = dst.read_bytes().partition(b"\n")
    w, h = (int(v) for v in head.split())
    return 0, 0, np.frombuffer(px, np.uint8).reshape(h, w, 3)


@pytest.fixture(scope="module")
def families():
    return {"a": jpeg_craft.family_a(), "b": jpeg_craft.family_b(), "c": jpeg_craft.family_c()}


def test_the_writer_writes_what_it_is_told(families):
    """PIL opens every file of A and B without a warning and with the size that was written; the parser reports the fields."""
    for name, data in families["a"] + families["b"]:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with Image.open(io.BytesIO(data)) as im:
                im.load()
                f = jpeg.parse(data)
                assert f.reason == 0 and (f.width, f.height) == im.size, name
                assert im.mode == ("L" if f.ncomp == 1 else "RGB"), name
    by_name = dict(families["a"])
    for (h, v) in ((1, 1), (2, 1), (2, 2)):
        for interval in (0, 2):
            f = jpeg.parse(by_name["a selectors %dx%d dri%d" % (h, v, interval)])
            assert (f.width, f.height, f.ncomp, f.restart_interval) == (37, 21, 3, interval)
            assert [(f.h[c], f.v[c]) for c in range(3)] == [(h, v), (1, 1), (1, 1)]
            assert [(f.tq[c], f.td[c], f.ta[c]) for c in range(3)] == [(2, 2, 3), (3, 1, 0), (0, 3, 2)]
            assert list(f.quant_defined) == [1, 1, 1, 1] and list(f.huff_defined) == [1] * 8
    for n in (256, 257, 513):
        f = jpeg.parse(by_name["a strip %d units" % n])
        assert (f.width, f.height, f.ncomp, f.restart_interval) == (8, 8 * n, 1, 1)
        assert by_name["a strip %d units" % n].count(b"\xff\xd7") == (n - 1) // 8         # RST7 closes every eighth segment
    for interval in (1, 3, 271, 272, 300):
        f = jpeg.parse(by_name["a grey 128x136 dri%d" % interval])
        assert (f.width, f.height, f.restart_interval) == (128, 136, interval)
    f = jpeg.parse(by_name["a grey sampled 2x2"])
    assert (f.ncomp, f.h[0], f.v[0]) == (1, 1, 1)                                         # the parser normalises a lone component
    assert by_name["a grey sampled 2x2"][by_name["a grey sampled 2x2"].index(b"\xff\xc0") + 11] == 0x22
    f = jpeg.parse(by_name["a 16-bit codes"])
    assert list(f.huff_counts[4]) == [1] + [0] * 14 + [255]
    f = jpeg.parse(by_name["a 420 272x256 dri1"])
    assert (f.width, f.height, f.restart_interval, f.h[0], f.v[0]) == (272, 256, 1, 2, 2)


def test_encodable_is_the_forward_dct():
    """A flat block has only its DC, 8 * (value - 128); a constant quantiser divides it."""
    c = jpeg_craft.encodable(np.full((8, 16), 255), 1)
    assert c.shape == (1, 2, 64) and (c[..., 0] == 1016).all() and not c[..., 1:].any()
    assert (jpeg_craft.encodable(np.zeros((8, 8)), 8)[..., 0] == -128).all()
    ramp = np.tile(np.arange(8) * 30, (8, 1))
    assert not jpeg_craft.encodable(ramp, 1)[0, 0].reshape(8, 8)[1:].any()                # constant along y: no vertical frequency


@pytest.mark.parametrize("family", ["a", "b"])
def test_what_an_encoder_can_write_decodes_to_pils_pixels(checker, tmp_path, families, family):
    wrong = []
    for name, data in families[family]:
        reason, status, px = host_decode(checker, tmp_path, data)
        if (reason, status) != (0, 0):
            wrong.append((name, reason, status))
        elif not np.array_equal(px, pil_rgb(data)):
            wrong.append((name, "pixels", int((px != pil_rgb(data)).any(-1).sum())))
    assert not wrong, wrong


MUST_BE_RANGE = jpeg_craft.C_MUST_BE_RANGE


def test_free_coefficients_are_refused_or_pils(checker, tmp_path, families):
    names = [n for n, _ in families["c"]]
    assert len(names) == 3 * len(jpeg_craft.C_PAIRS) + 4 and set(MUST_BE_RANGE) <= set(names)
    wrong, statuses = [], {}
    for name, data in families["c"]:
        reason, status, px = host_decode(checker, tmp_path, data)
        assert reason == 0, name                                                         # well-formed files: the parser takes them
        statuses[name] = status
        if status == 0 and not np.array_equal(px, pil_rgb(data)):
            wrong.append((name, int((px != pil_rgb(data)).any(-1).sum())))
    assert not wrong, wrong
    assert {n: statuses[n] for n in MUST_BE_RANGE} == {n: _ffi.JPEG_S_RANGE for n in MUST_BE_RANGE}
    assert set(statuses.values()) <= {0, _ffi.JPEG_S_RANGE}
    assert statuses["c q1 A64 n1"] == 0 and statuses["c q1 A64 n4"] == 0 and statuses["c q1 A64 n64"] == 0


@pytest.mark.parametrize("which", [0, 1, 2])
def test_single_byte_corruptions_are_refused_or_pils(checker, tmp_path, which):
    """Status 0 means PIL's bytes, also for a damaged file: 300 seeded single-byte corruptions of the scan.  Where PIL raises,
    the status is not 0.  At least 10 % decode with status 0, so the promise is not kept by refusing everything."""
    name, good = jpeg_craft.corruption_sources()[which]
    reason, status, px = host_decode(checker, tmp_path, good)
    assert (reason, status) == (0, 0) and np.array_equal(px, pil_rgb(good))
    decoded, wrong = 0, []
    for i, data in enumerate(jpeg_craft.corruptions(good, 300, jpeg_craft.CORRUPTION_SEEDS[which])):
        reason, status, px = host_decode(checker, tmp_path, data)
        if reason or status:
            continue
        decoded += 1
        try:
            ref = evaluate.read_image_rgb(io.BytesIO(data))
        except Exception as e:
            wrong.append((i, "PIL raises", repr(e)[:80]))
            continue
        if ref.shape != px.shape or not np.array_equal(px, ref):
            wrong.append((i, "pixels", int((px != ref).any(-1).sum()) if ref.shape == px.shape else ref.shape))
    print("%s: %d of 300 corruptions decode with status 0" % (name, decoded))
    assert not wrong, wrong
    assert decoded >= 30, decoded
