"""The host side of the draw stage, no GPU: rectangle rounding, the label atlas' shapes and bit order, the palette, the struct
layouts, the argument checks of ``yv3_draw_boxes`` and the numpy pixel rule (tests/draw_ref.py) on cases small enough to read."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_ref  # noqa: E402
from yolo_v3_amd import _ffi, draw  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rectangles_round_half_to_even_in_float64():
    got = draw.rectangles([[0.5, 1.5, 2.0, 2.0], [-0.5, -1.5, 10.25, 3.0], [3.49999, 2.50001, 0.0, 0.0]])
    assert got.dtype == np.int32
    assert got.tolist() == [[0, 2, 2, 4], [0, -2, 10, 2], [3, 3, 3, 3]]                 # np.rint: halves go to the even neighbour
    assert draw.rectangles(np.zeros((0, 4))).shape == (0, 4)
    x = np.float32(16777217.0)                                                          # the sum is taken in float64, not float32
    assert draw.rectangles(np.array([[x, 0, 1, 0]], np.float32))[0, 2] == int(x) + 1


def test_atlas_shapes_and_bit_order():
    masks = [np.array([[1, 0, 0, 0, 0, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 0, 0, 0, 1, 1]], bool), np.ones((3, 8), bool), np.zeros((1, 1), bool)]
    atlas = draw.LabelAtlas(masks=masks)
    assert atlas.records == [(0, 10, 2), (4, 8, 3), (7, 1, 1)]                          # rows of ceil(mw / 8) bytes, back to back
    assert atlas.data.tolist() == [0x80, 0x40, 0x40, 0xC0, 0xFF, 0xFF, 0xFF, 0x00]      # the leftmost pixel is bit 7
    names = ["person", "x-wing", "tie fighter", ""]
    atlas = draw.LabelAtlas(names)
    assert len(atlas) == 4
    for name, m, (off, mw, mh) in zip(names, atlas.masks, atlas.records):
        assert m.dtype == bool and m.shape == (mh, mw) and (m.any() == bool(name))
        assert not m[0].any() and not m[-1].any() and not m[:, 0].any() and not m[:, -1].any()     # the margin is clear
        rows = atlas.data[off:off + mh * ((mw + 7) // 8)].reshape(mh, -1)
        assert np.array_equal(np.unpackbits(rows, axis=1)[:, :mw].astype(bool), m)
    assert np.array_equal(draw.rasterise("person"), atlas.masks[0])                     # rasterising is repeatable


def test_palette_is_fixed_and_distinct():
    p = draw.palette(80)
    assert p.dtype == np.uint8 and p.shape == (80, 3)
    assert len({tuple(c) for c in p.tolist()}) == 80 and (0, 0, 0) not in {tuple(c) for c in p.tolist()}
    assert np.array_equal(draw.palette(255)[:80], p) and len({tuple(c) for c in draw.palette(255).tolist()}) == 255
    assert p[:3].tolist() == [[128, 0, 0], [0, 128, 0], [128, 128, 0]]


@pytest.mark.parametrize("ctype,cname", [(_ffi.DrawImage, "yv3_draw_image"), (_ffi.DrawBox, "yv3_draw_box"), (_ffi.DrawTag, "yv3_draw_tag")])
def test_struct_layouts_match_the_c_header(tmp_path, ctype, cname):
    fields = [f for f, _ in ctype._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv3.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % cname
                   + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields]


def test_draw_call_checks_its_arguments_before_launching():
    lib = _ffi.lib()
    ok = dict(images=4096, B=1, boxes=4096, n=1, tags=4096, ntags=1, atlas=4096, atlas_bytes=8, t=1, mw=8, mh=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.yv3_draw_boxes(a["images"], a["B"], a["boxes"], a["n"], a["tags"], a["ntags"], a["atlas"], a["atlas_bytes"], a["t"], a["mw"],
                                  a["mh"], None)

    for bad in (dict(images=None), dict(B=0), dict(boxes=None), dict(n=-1), dict(tags=None), dict(atlas=None), dict(t=0), dict(mw=0),
                dict(mh=0), dict(atlas_bytes=-1)):
        assert call(**bad) == _ffi.EINVAL, bad
    assert call(n=0, boxes=None) == 0                                                   # nothing to draw: nothing is launched


def test_pixel_rule_on_readable_cases():
    img = np.full((6, 7, 3), 9, np.uint8)
    red, blue = (200, 0, 0), (0, 0, 200)
    out = draw_ref.draw(img, [[1, 1, 5, 4]], [red], thickness=1)
    want = np.zeros((6, 7), bool)
    want[1, 1:6] = want[4, 1:6] = want[1:5, 1] = want[1:5, 5] = True
    assert np.array_equal((out == red).all(-1), want) and (out[~want] == 9).all()
    assert np.array_equal(draw_ref.draw(img, [[1, 1, 5, 4]], [red], thickness=2), draw_ref.draw(img, [[1, 1, 5, 4]], [red], thickness=9))
    assert (draw_ref.draw(img, [[1, 1, 5, 4]], [red], thickness=2)[1:5, 1:6] == red).all()       # t above half the box: filled
    one = draw_ref.draw(img, [[3, 2, 3, 2]], [red], thickness=1)                                # a zero-area box is one pixel
    assert (one[2, 3] == red).all() and int((one != img).any(-1).sum()) == 1
    assert np.array_equal(draw_ref.draw(img, [[5, 4, 1, 1]], [red]), img)                        # corners the wrong way round: nothing
    assert np.array_equal(draw_ref.draw(img, [[-9, -9, -2, -2], [7, 6, 20, 20]], [red, blue]), img)
    both = draw_ref.draw(img, [[0, 0, 3, 3], [2, 2, 6, 5]], [red, blue], thickness=1)
    assert (both[3, 3] == red).all() and (both[3, 2] == blue).all() and (both[2, 3] == blue).all()   # the later box wins, where it paints
    mask = np.array([[1, 0, 1], [0, 1, 0]], bool)
    tagged = draw_ref.draw(img, [[2, 3, 2, 3]], [red], tags=[0], masks=[mask], thickness=1)
    assert (tagged[1:3, 2:5].reshape(-1, 3) == [[0] * 3, red, [0] * 3, red, [0] * 3, red]).all()   # the tag sits above y1, at x1
    top = draw_ref.draw(img, [[6, 0, 6, 0]], [red], tags=[0], masks=[mask], thickness=1)         # clipped: right edge, top edge
    assert (top[0:2, 4:7].reshape(-1, 3) == [[0] * 3, red, [0] * 3, red, [0] * 3, red]).all()
    narrow = draw_ref.draw(img[:, :2], [[0, 5, 0, 5]], [red], tags=[0], masks=[mask], thickness=1)   # an image narrower than the mask
    assert (narrow[3:5].reshape(-1, 3) == [[0] * 3, red, red, [0] * 3]).all()
