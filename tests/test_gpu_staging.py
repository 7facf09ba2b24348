"""The three augmentation stages on one staged-batch helper (yolo_v3_amd/_staging.py): the same bits from host arrays and from views
into one allocation, and every stage's upload counted as the layout function (held to a restatement in tests/test_staging_host.py)
gives it."""
import numpy as np
import pytest
import torch

from yolo_v3_amd import _staging
from yolo_v3_amd import affine_augment as affine
from yolo_v3_amd import augment as aug
from yolo_v3_amd import extra_augment as extra

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_stages_count_the_layouts_upload_and_agree_across_entrances():
    shapes, B, dim = [(5, 7), (3, 85)], 2, (64, 64)
    rng = np.random.RandomState(3)
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    labels = [np.array([[1, 0.5, 0.5, 0.4, 0.6], [2, 0.3, 0.6, 0.2, 0.3]]), np.array([[0, 0.5, 0.5, 0.5, 0.8]])]
    warps = affine.sample_affine(range(B), shapes, p=1.0)
    programs = extra.sample_extra(range(B), shapes)
    params = aug.sample_params(range(B), shapes=shapes)
    arena = torch.empty(2048, dtype=torch.uint8, device=DEV)
    views = [arena[at:at + im.size].view(im.shape) for at, im in zip((256, 1024), imgs)]
    for v, im in zip(views, imgs):
        v.copy_(torch.from_numpy(im))

    def upload(records_bytes, label_bytes, host):
        return _staging.layout(shapes, records_bytes, label_bytes, [host] * B, not host).upload

    results = []
    for sources, host in ((imgs, True), (views, False)):
        seen = [dict(aug.counters)]
        warped, rows = affine.affine_augment_batch(sources, labels, warps)
        seen.append(dict(aug.counters))
        blurred = extra.extra_augment_batch(warped, programs)
        seen.append(dict(aug.counters))
        x, target = aug.augment_batch(blurred, rows, dim, params)
        seen.append(dict(aug.counters))
        # the list's two rows and one row go up padded (2 x 2 x 40 bytes); the later stages gather device images and labels
        expect = [upload(affine.PROGRAM.itemsize * B, 40 * 2 * B, host), upload(extra.PROGRAM.itemsize * B, 0, False),
                  upload(8 * aug.N_PARAMS * B, 0, False)]
        assert [b["upload_bytes"] - a["upload_bytes"] for a, b in zip(seen, seen[1:])] == expect
        assert [b["batches"] - a["batches"] for a, b in zip(seen, seen[1:])] == [0, 0, 1]
        results.append((warped, rows, blurred, x, target))
    a, b = results
    assert all(torch.equal(p, q) for p, q in zip(a[0] + a[2], b[0] + b[2]))
    assert torch.equal(a[1].view(torch.int64), b[1].view(torch.int64)) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert tuple(a[1].shape) == (B, 2, 5) and a[4].any().item()
    assert all(np.array_equal(v.cpu().numpy(), im) for v, im in zip(views, imgs))
