"""`draw.draw_boxes` on the GPU against the numpy pixel rule (tests/draw_ref.py), bit for bit, on images of 40x56 and 17x33."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_ref  # noqa: E402
from yolo_v3_amd import draw  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["person", "x-wing", "a much longer label than the image is wide", "i"]
ATLAS = draw.LabelAtlas(NAMES)
COLORS = draw.palette(8)


def image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def check(images, rects, tags, thickness):
    """One call for the batch; every image against the reference."""
    colors = [COLORS[np.arange(len(r)) % len(COLORS)] for r in rects]
    dev = [torch.from_numpy(a).cuda() for a in images]
    got = draw.draw_boxes(dev, rects, colors, tags, ATLAS if tags is not None else None, thickness=thickness)
    torch.cuda.synchronize()
    for i, a in enumerate(images):
        want = draw_ref.draw(a, rects[i], colors[i], None if tags is None else tags[i], ATLAS.masks, thickness)
        assert np.array_equal(got[i].cpu().numpy(), want), i
    return [g.cpu().numpy() for g in got]


# (width, height) = (40, 56) and (17, 33); every list is one image's boxes, x1 y1 x2 y2
CASES = {
    "overlapping boxes": [[[4, 20, 30, 44], [10, 26, 38, 50], [2, 30, 20, 54]], [[1, 12, 12, 28], [5, 14, 16, 30]]],
    "partly and wholly outside": [[[-10, -5, 12, 30], [30, 40, 70, 90], [-50, -50, -3, -3], [41, 0, 60, 20], [0, 56, 39, 80]],
                                  [[-4, 20, 30, 40], [17, 33, 20, 36], [-3, -3, 20, 36]]],
    "zero area": [[[20, 30, 20, 30], [0, 0, 0, 0], [39, 55, 39, 55]], [[8, 20, 8, 20], [16, 32, 16, 32]]],
    "corners the wrong way round": [[[30, 44, 4, 20]], [[12, 28, 1, 12]]],
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("tagged", [False, True])
def test_boxes_equal_the_reference(name, tagged):
    rects = [np.array(r, np.int32) for r in CASES[name]]
    tags = [np.arange(len(r)) % 2 for r in rects] if tagged else None
    out = check([image(40, 56, 1), image(17, 33, 2)], rects, tags, 2)
    if name == "corners the wrong way round" and not tagged:
        assert np.array_equal(out[0], image(40, 56, 1))


@pytest.mark.parametrize("thickness", [1, 3, 7, 100])
def test_thickness_up_to_more_than_half_the_box(thickness):
    check([image(40, 56, 3), image(17, 33, 4)], [np.array([[5, 20, 17, 31], [20, 22, 38, 50]], np.int32), np.array([[2, 14, 14, 20]], np.int32)],
          None, thickness)


def test_tags_clipped_at_the_left_right_and_top_edges():
    mw, mh = ATLAS.records[0][1], ATLAS.records[0][2]
    assert mw < 40 and mh < 56 and ATLAS.records[2][1] > 40 > 17                      # the long label is wider than both images
    rects = [np.array([[-8, 30, 10, 40],                                                # x1 < 0: the tag starts at column 0
                       [36, 30, 39, 45],                                                # x1 + mw > W: the tag is pushed left
                       [10, 3, 30, 20],                                                 # y1 < mh: the tag starts at row 0, below y1
                       [12, 50, 30, 55]], np.int32),
             np.array([[2, 16, 15, 30], [0, 2, 16, 10]], np.int32)]
    tags = [np.array([0, 0, 1, 3]), np.array([2, 2])]                                   # 17 wide: an image narrower than its mask
    out = check([image(40, 56, 5), image(17, 33, 6)], rects, tags, 1)
    assert (out[0][30 - mh:30, 0:mw] != image(40, 56, 5)[30 - mh:30, 0:mw]).any()
    assert (out[1][16 - ATLAS.records[2][2]:16, :] != image(17, 33, 6)[16 - ATLAS.records[2][2]:16, :]).any(-1).all()      # cropped to the full width


def test_an_image_without_boxes_is_untouched_and_sizes_mix():
    a, b, c = image(40, 56, 7), image(17, 33, 8), image(40, 56, 9)
    none = np.zeros((0, 4), np.int32)
    out = check([a, b, c], [none, np.array([[3, 12, 12, 25]], np.int32), none], [np.zeros(0, np.int32), np.array([1]), np.zeros(0, np.int32)], 2)
    assert np.array_equal(out[0], a) and np.array_equal(out[2], c) and not np.array_equal(out[1], b)
    out = check([a, b], [none, none], None, 2)                                          # no box in the whole batch: no launch at all
    assert np.array_equal(out[0], a) and np.array_equal(out[1], b)


def test_pitched_rows_and_many_boxes():
    big = torch.from_numpy(image(64, 60, 10)).cuda()
    view = big[2:58, 12:52]                                                             # 40 x 56 inside 64 x 60
    before = big.clone()
    rng = np.random.RandomState(11)
    x, y = rng.randint(-10, 45, 40), rng.randint(-10, 60, 40)
    rects = np.stack([x, y, x + rng.randint(0, 30, 40), y + rng.randint(0, 30, 40)], 1).astype(np.int32)
    tags = rng.randint(-1, 4, 40)
    colors = COLORS[np.arange(40) % 8]
    draw.draw_boxes([view], [rects], [colors], [tags], ATLAS, thickness=2)
    torch.cuda.synchronize()
    want = draw_ref.draw(before[2:58, 12:52].cpu().numpy(), rects, colors, tags, ATLAS.masks, 2)
    assert np.array_equal(view.cpu().numpy(), want)
    outside = torch.ones_like(big, dtype=torch.bool)
    outside[2:58, 12:52] = False
    assert torch.equal(big[outside], before[outside])                                   # nothing outside the view was written


def test_arguments_the_wrapper_refuses():
    im = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    one = [np.array([[1, 1, 4, 4]], np.int32)]
    with pytest.raises(ValueError):
        draw.draw_boxes([im], one, [COLORS[:1]], thickness=0)
    with pytest.raises(ValueError):
        draw.draw_boxes([im], one, [COLORS[:2]])
    with pytest.raises(ValueError):
        draw.draw_boxes([im], one, [COLORS[:1]], [np.array([4])], ATLAS)
    with pytest.raises(Exception):
        draw.draw_boxes([im.float()], one, [COLORS[:1]])
    with pytest.raises(Exception):
        draw.draw_boxes([im.cpu()], one, [COLORS[:1]])
