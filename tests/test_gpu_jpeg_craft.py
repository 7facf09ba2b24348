"""The GPU JPEG decoder on files PIL's encoder does not write (tests/jpeg_craft.py) and on damaged files with a pixel check,
against PIL's decode of the same bytes in the same process.  tests/test_jpeg_craft_host.py runs the same inputs through the
same headers on the CPU under ASan + UBSan first; every input here ends in a status by the bounded bit reader.

What runs here and nowhere else in the suite: `entropy_kernel`'s unit loop beyond its first trip (256, 257 and 513 restart
segments), the marker count, its prefix and ``marks[k]`` for k >= 256, the ``u & 7`` marker check over 64 wraps, Huffman
selectors and quantiser tables 2 and 3, SOF1, other component ids, `idct_kernel` raising YV3_JPEG_S_RANGE, and
`colour_kernel`'s grid-stride loop (more than 4096 x 256 groups of 4 pixels).  `idct_kernel`'s own stride loop needs more than
1 048 576 blocks (a 67 MP image) and is left out on purpose."""
import io

import numpy as np
import pytest
import torch

from tests import jpeg_abi, jpeg_craft
from yolo_v3_amd import _ffi, evaluate, jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = jpeg_abi.FILL


def pil_rgb(data):
    return evaluate.read_image_rgb(io.BytesIO(data))


def test_families_a_and_b_in_one_mixed_batch_through_the_c_abi():
    """Everything an encoder can write, crafted and PIL-written, in one batch: every status 0, every image PIL's."""
    cases = jpeg_craft.family_a() + jpeg_craft.family_b()
    assert len(cases) >= 70
    r = jpeg_abi.decode([d for _, d in cases])
    bad = [(name, int(s)) for (name, _), s in zip(cases, r.statuses) if s]
    assert not bad, bad
    wrong = []
    for (name, data), px in zip(cases, r.images):
        ref = pil_rgb(data)
        if px.size != ref.size or not np.array_equal(px.reshape(ref.shape), ref):
            wrong.append(name)
    assert not wrong, wrong


def check_against_read_image_rgb(names, datas):
    """`decode_batch(errors="keep")` of ``datas``: every result is `read_image_rgb`'s pixels or its exception, ``fallback`` is
    true exactly where ``reasons`` is set, one upload and one status read for the call.  Returns the `Decoded` list."""
    before = dict(jpeg.counters)
    out = jpeg.decode_batch(datas, device=DEV, errors="keep")
    spent = {k: jpeg.counters[k] - before[k] for k in ("calls", "uploads", "status_reads", "fallbacks")}
    assert spent == {"calls": 1, "uploads": 1, "status_reads": 1, "fallbacks": sum(out.fallback)}
    assert len(out) == len(datas) and out.fallback == [r is not None for r in out.reasons]
    wrong = []
    for name, data, got, reason in zip(names, datas, out, out.reasons):
        try:
            ref = pil_rgb(data)
        except Exception as e:
            if reason is None or type(got) is not type(e) or str(got) != str(e):
                wrong.append((name, reason, "PIL raises %r" % e))
            continue
        if isinstance(got, Exception) or tuple(got.shape) != ref.shape or not np.array_equal(got.cpu().numpy(), ref):
            wrong.append((name, reason, "pixels"))
    assert not wrong, wrong
    return out


def test_free_coefficients_come_back_as_pil_gives_them():
    cases = jpeg_craft.family_c()
    out = check_against_read_image_rgb([n for n, _ in cases], [d for _, d in cases])
    reasons = dict(zip([n for n, _ in cases], out.reasons))
    assert {n: reasons[n] for n in jpeg_craft.C_MUST_BE_RANGE} == {n: ("device", _ffi.JPEG_S_RANGE) for n in jpeg_craft.C_MUST_BE_RANGE}
    assert set(reasons.values()) <= {None, ("device", _ffi.JPEG_S_RANGE)}
    assert reasons["c q1 A64 n64"] is None and reasons["c q1 A64 n1"] is None


@pytest.mark.parametrize("which", [0, 1, 2])
def test_single_byte_corruptions_come_back_as_pil_gives_them(which):
    """The first 60 of the host test's 300 corruptions of each file, in one call; at least one is decoded on the device."""
    name, good = jpeg_craft.corruption_sources()[which]
    datas = [good] + jpeg_craft.corruptions(good, 60, jpeg_craft.CORRUPTION_SEEDS[which])
    out = check_against_read_image_rgb(["%s #%d" % (name, i) for i in range(len(datas))], datas)
    assert out.reasons[0] is None
    assert out.fallback[1:].count(False) >= 1 and out.fallback[1:].count(True) >= 1, out.reasons


def test_a_refused_block_between_good_neighbours_through_the_c_abi():
    """good, RANGE, good: the neighbours are PIL's, the refused image's destination keeps its fill value."""
    c = dict(jpeg_craft.family_c())
    good_a, refused, good_b = c["c q1 A64 n64"], c["c q8 A1023 n64"], c["c q1 A256 n4"]
    r = jpeg_abi.decode([good_a, refused, good_b])
    statuses, images = r.statuses.tolist(), r.images
    assert statuses == [0, _ffi.JPEG_S_RANGE, 0]
    assert np.array_equal(images[0].reshape(48, 48, 3), pil_rgb(good_a)) and np.array_equal(images[2].reshape(48, 48, 3), pil_rgb(good_b))
    assert images[1].size == 48 * 48 * 3 and (images[1] == FILL).all()


def test_the_colour_kernels_grid_stride_loop():
    """A flat 2048x2064 grey file (PIL-written, about 50 KB), alone in a batch: 1 056 768 groups of four pixels, above the
    4096 x 256 lanes of `colour_kernel`'s largest grid."""
    data = jpeg_craft.pil_bytes(np.full((2064, 2048), 77, np.uint8), quality=75)
    assert len(data) < 64 * 1024 and 2048 * 2064 // 4 > 4096 * 256
    ref = pil_rgb(data)
    out = jpeg.decode_batch([data], device=DEV)
    assert out.fallback == [False] and tuple(out[0].shape) == (2064, 2048, 3)
    assert torch.equal(out[0].cpu(), torch.from_numpy(ref))
    # the same size with another grey level in every 8x8 block (85 KB): a pixel written to the wrong place shows
    yy, xx = np.mgrid[0:2064, 0:2048]
    data = jpeg_craft.pil_bytes(((xx // 8) * 7 + (yy // 8) * 13) % 256, quality=75)
    out = jpeg.decode_batch([data], device=DEV)
    assert out.fallback == [False] and torch.equal(out[0].cpu(), torch.from_numpy(pil_rgb(data)))
