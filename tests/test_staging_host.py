"""The host half the augmentation stages share (yolo_v3_amd/_staging.py) without a GPU: the staged buffer's layout against a
restatement written out here, the label padding and the image checks."""
import numpy as np
import pytest
import torch

from yolo_v3_amd import _ffi, _staging
from yolo_v3_amd import affine_augment as affine
from yolo_v3_amd import augment as aug
from yolo_v3_amd import extra_augment as extra

BATCHES = [[(1, 1)], [(1, 1), (5, 7), (3, 85)]]              # 3 H W of the second: 3, 105 (below 256), 765 (above); 256-aligned sums on it
RECORDS = {"params": 64, "extra": extra.PROGRAM.itemsize, "affine": affine.PROGRAM.itemsize}
MODES = ["host", "device", "mixed", "gather"]


def up(n):
    return (n + 255) // 256 * 256


def restated(shapes, records_bytes, label_bytes, on_host, gather):
    """records | offsets | hw | labels | [gather: source offsets] or [images], every section and every image on a multiple of 256."""
    B = len(shapes)
    start, pos = {}, 0
    for name, n in [("records", records_bytes), ("offsets", 8 * B), ("hw", 8 * B), ("labels", label_bytes)]:
        start[name] = pos
        pos = up(pos + n)
    start["images"] = pos
    image_at, span = [], 0
    for h, w in shapes:
        image_at.append(span)
        span = up(span + 3 * h * w)
    if gather:
        total = upload = pos + 8 * B
    elif any(on_host):
        total = upload = pos + span
    else:
        total, upload = pos + span, pos
    return start, image_at, span, total, upload


def on_host(mode, B):
    return {"host": [True] * B, "device": [False] * B, "gather": [False] * B, "mixed": [b % 2 == 0 for b in range(B)]}[mode]


@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("records", sorted(RECORDS))
@pytest.mark.parametrize("shapes,mode", [(s, m) for s in BATCHES for m in MODES if len(s) > 1 or m != "mixed"],    # one image cannot be mixed
                         ids=lambda v: v if isinstance(v, str) else "B%d" % len(v))
def test_layout(shapes, mode, records, rows):
    B = len(shapes)
    rec, lab, host, gather = RECORDS[records] * B, 40 * rows * B, on_host(mode, B), mode == "gather"
    L = _staging.layout(shapes, rec, lab, host, gather)
    start, image_at, span, total, upload = restated(shapes, rec, lab, host, gather)
    assert (0, L.o_off, L.o_hw, L.o_lab, L.o_img) == tuple(start[k] for k in ("records", "offsets", "hw", "labels", "images"))
    assert (list(L.offsets), L.span, L.total, L.upload) == (image_at, span, total, upload)

    # aligned, in order, disjoint
    sections = [(0, rec), (L.o_off, 8 * B), (L.o_hw, 8 * B), (L.o_lab, lab)]
    if gather:
        sections.append((L.o_img, 8 * B))
    else:
        sections += [(L.o_img + off, 3 * h * w) for off, (h, w) in zip(L.offsets, shapes)]
    assert all(at % 256 == 0 for at, _ in sections)
    assert all(a + n <= b for (a, n), (b, _) in zip(sections, sections[1:]))
    assert sections[-1][0] + sections[-1][1] <= L.total and L.total - (sections[-1][0] + sections[-1][1]) < 256
    # the three upload rules
    if gather:
        assert L.upload == L.total == L.o_img + 8 * B
    elif any(host):
        assert L.upload == L.total == L.o_img + L.span
    else:
        assert L.upload == L.o_img and L.total == L.o_img + L.span
    # a stage without labels (programs | offsets | hw | images) is the stage with a label section of no bytes
    if lab == 0:
        assert L.o_lab == L.o_img == up(L.o_hw + 8 * B)


def test_records_sizes_are_the_stages_own():
    assert RECORDS["params"] == aug.N_PARAMS * 8 and RECORDS["extra"] % 8 == 0 and RECORDS["affine"] == 104
    assert aug.counters is _staging.counters and set(aug.counters) == {"batches", "upload_bytes"}


# ---- pad_labels ---------------------------------------------------------------------------------------------------------------
def test_pad_labels_none():
    assert _staging.pad_labels(None, 3) == (None, None, 0)


def test_pad_labels_lists():
    rng = np.random.RandomState(0)
    a, b = rng.rand(2, 5), rng.rand(3, 5).astype(np.float32)
    dev, host, T = _staging.pad_labels([a, np.zeros((0, 5)), b], 3)
    assert dev is None and T == 3 and host.dtype == np.float64 and host.shape == (3, 3, 5)
    assert np.array_equal(host[0, :2], a) and np.array_equal(host[2], b.astype(np.float64))
    assert not host[0, 2:].any() and not host[1].any()
    dev, host, T = _staging.pad_labels([[], []], 2)          # nothing but empty entries: a label section of no bytes
    assert dev is None and T == 0 and host.shape == (2, 0, 5) and host.nbytes == 0


def test_pad_labels_cpu_tensor_becomes_float64():
    t = torch.arange(2 * 3 * 5, dtype=torch.float32).reshape(2, 3, 5)
    dev, host, T = _staging.pad_labels(t, 2)
    assert dev is None and T == 3 and isinstance(host, np.ndarray) and host.dtype == np.float64
    assert np.array_equal(host, t.numpy().astype(np.float64))


def test_pad_labels_refusals():
    with pytest.raises(ValueError, match=r"^one label array per image$"):
        _staging.pad_labels([np.zeros((1, 5))], 2)
    with pytest.raises(ValueError, match=r"^padded labels must be \[B,T,5\]$"):
        _staging.pad_labels(torch.zeros(3, 2, 5), 2)
    with pytest.raises(ValueError, match=r"^padded labels must be \[B,T,5\]$"):
        _staging.pad_labels(torch.zeros(2, 2, 4), 2)
    with pytest.raises(ValueError, match=r"^padded labels must be \[B,T,5\]$"):
        _staging.pad_labels(torch.zeros(2, 5), 2)


# ---- as_images ----------------------------------------------------------------------------------------------------------------
def test_as_images(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    a, t = np.zeros((5, 7, 3), np.uint8), torch.zeros((3, 85, 3), dtype=torch.uint8)
    imgs, shapes = _staging.as_images([a[:, ::-1], t])       # a numpy view is made contiguous, a tensor is taken as it is
    assert shapes == [(5, 7), (3, 85)] and imgs[1] is t and imgs[0].dtype == torch.uint8 and imgs[0].is_contiguous()
    for bad in (np.zeros((5, 7, 3), np.float32), np.zeros((5, 7), np.uint8), np.zeros((5, 7, 4), np.uint8),
                np.zeros((0, 7, 3), np.uint8), torch.zeros((5, 0, 3), dtype=torch.uint8)):
        with pytest.raises(_ffi.Yv3Error, match=r"^images must be uint8 \[H,W,3\] RGB$"):
            _staging.as_images([a, bad])
    with pytest.raises(ValueError, match=r"^empty batch$"):
        _staging.as_images([])


def test_no_gpu_is_said_first(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for images in ([], [np.zeros((5, 7), np.float32)]):
        with pytest.raises(_ffi.Yv3Error, match=r"^no GPU available: this package has no CPU path$"):
            _staging.as_images(images)
