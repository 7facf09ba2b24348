"""`evaluate.annotate_images` end to end on tests/golden/x_wing_0001.jpg with synthetic weights: the written file equals PIL's
encoding of the numpy drawing rule (tests/draw_ref.py) applied to the decoded image with the boxes the run drew."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_ref  # noqa: E402
import jpeg_enc_ref as ref  # noqa: E402
from helpers import load_sw1_net  # noqa: E402
from yolo_v3_amd import draw, evaluate, jpeg, synth  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHOTO = os.path.join(REPO, "tests", "golden", "x_wing_0001.jpg")
NAMES = ["c%d" % i for i in range(80)]
CONF = 0.05         # these synthetic weights give the photograph 100 boxes at 0.05 and none at 0.3


@pytest.fixture(scope="module")
def net():
    return load_sw1_net(synth.weight_stream(b_obj=-1.0, b_cls=-4.0), size=96).cuda()


@pytest.mark.parametrize("decode", ["pil", "gpu"])
def test_annotated_file_equals_pil_of_the_reference_drawing(net, tmp_path, decode):
    before = dict(jpeg.counters)
    writer = evaluate.annotate_images(net, [PHOTO], NAMES, str(tmp_path / "out"), 2, (96, 96), is_letterbox=True, decode=decode,
                                      obj_conf_thr=CONF, nms_thr=0.4, quality=75)
    assert writer.written == [str(tmp_path / "out" / "x_wing_0001.jpg")]
    rects, classes = writer.boxes[0]
    print("boxes drawn: %d" % len(rects))
    assert len(rects) >= 1, "no box at this threshold: nothing would be compared"
    pixels = evaluate.read_image_rgb(PHOTO)
    atlas = draw.LabelAtlas(NAMES)
    want = draw_ref.draw(pixels, rects, draw.palette(80)[classes], classes, atlas.masks, 2)
    assert not np.array_equal(want, pixels)
    with open(writer.written[0], "rb") as f:
        assert f.read() == ref.pil_file(want, 75, "4:2:0")
    if decode == "gpu":                                             # decoded on the device, never handed to PIL, nothing uploaded to encode
        assert jpeg.counters["fallbacks"] == before["fallbacks"] and jpeg.counters["uploads"] == before["uploads"] + 1
