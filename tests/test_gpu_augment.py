"""The training augmentation on the GPU (yolo_v3_amd/augment.py, csrc/augment.hip) against the numpy restatement tests/augment_ref.py:
identical pixels, the same kept label rows (values within 1e-6), the existing letterbox kernel as a cross-check, a training step on
the output, determinism, bounds, error codes and the list-file loader."""

import numpy as np
import pytest
import torch

from tests import augment_ref as A
from tests.helpers import trained_like_stream
from yolo_v3_amd import YoloNet, WeightManager, _ffi, letterbox_batch
from yolo_v3_amd import augment as aug

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(480, 640), (333, 501), (1231, 97), (97, 1231), (100, 150), (832, 832), (1, 1), (37, 1), (2, 3)]


def images(shapes, seed):
    rng = np.random.RandomState(seed)
    out = []
    for (h, w) in shapes:
        # smooth colour ramps plus noise: every hue sector and the grey axis occur
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 97) % 256], -1)
        out.append(np.clip(base + rng.randint(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


def extreme_params(shapes, k):
    """Parameter rows at the ends of darknet's ranges: every side -0.3 or +0.3, dsat / dexp at 1/1.5 and 1.5, |dhue| = 17.9, flips."""
    rows = []
    for i, (h, w) in enumerate(shapes):
        j = i + k
        sgn = [1 if (j >> b) & 1 else -1 for b in range(4)]
        sides = [np.rint(0.3 * n) * s for n, s in zip((h, w, h, w), sgn)]
        sides[0], sides[2] = aug.keep_one_pixel(sides[0], sides[2], h)
        sides[3], sides[1] = aug.keep_one_pixel(sides[3], sides[1], w)
        rows.append([17.9 if j % 2 else -17.9, 1.5 if j % 3 else 1 / 1.5, 1 / 1.5 if j % 4 < 2 else 1.5] + sides + [float(j % 2)])
    return np.array(rows, dtype=np.float64)


def run(imgs, labels, dim, params):
    x, t = aug.augment_batch(imgs, labels, dim, params)
    torch.cuda.synchronize()
    return x.cpu().numpy(), t.cpu().numpy()


@pytest.mark.parametrize("dim", [(416, 416), (608, 608), (416, 288)])
@pytest.mark.parametrize("kind", ["extreme", "sampled"])
def test_pixels_identical_to_restatement(dim, kind):
    imgs = images(SHAPES, 1)
    if kind == "extreme":
        params = extreme_params(SHAPES, dim[0] + dim[1])
    else:
        params = aug.sample_params(np.arange(len(SHAPES)) + dim[1], shapes=SHAPES)
    x, _ = run(imgs, None, dim, params)
    assert x.shape == (len(SHAPES), 3, dim[1], dim[0])
    for b, (img, p) in enumerate(zip(imgs, params)):
        ref = A.augment_image(img, p, dim)
        assert np.array_equal(x[b], ref), "image %d %s params %s: %d bytes differ" % (b, img.shape, p, int((x[b] != ref).sum()))


def test_identity_params_equal_the_eval_letterbox_of_the_roundtrip():
    imgs = images(SHAPES, 2)
    params = np.tile([0.0, 1.0, 1.0, 0, 0, 0, 0, 0], (len(imgs), 1))
    for dim in [(416, 416), (608, 352)]:
        x, _ = run(imgs, None, dim, params)
        for b, img in enumerate(imgs):
            lb, _ = letterbox_batch([A.hsv_roundtrip(img)], dim, variant="eval")
            assert np.array_equal(x[b], lb[0].cpu().numpy())


def test_crop_flip_equal_the_eval_letterbox_of_the_intermediate():
    imgs = images(SHAPES, 3)
    params = extreme_params(SHAPES, 1)
    x, _ = run(imgs, None, (416, 416), params)
    for b, (img, p) in enumerate(zip(imgs, params)):
        lb, _ = letterbox_batch([A.intermediate(img, p)], (416, 416), variant="eval")
        assert np.array_equal(x[b], lb[0].cpu().numpy())


# ---- labels -------------------------------------------------------------------------------------------------------------------
def label_rows(rng, n, C=80):
    r = np.zeros((n, 5))
    r[:, 0] = rng.randint(0, C, n)
    r[:, 1:3] = rng.uniform(-0.05, 1.05, (n, 2))             # some centres off the image: cut-out boxes
    r[:, 3:5] = rng.uniform(0.0, 0.6, (n, 2))
    r[rng.uniform(size=n) < 0.1, 3] = 0.0                    # degenerate rows
    return r


def off_threshold_rows(seed, n, H, W, p, dim, C=80):
    """Rows whose kept-area fraction is at least 1e-6 away from bbs_remove_cut_out's 0.1 (a tie would test rounding, not rules)."""
    for k in range(100):
        rng = np.random.RandomState(seed * 100 + k)
        rows = label_rows(rng, n, C)
        _, fracs = A.augment_labels(rows, H, W, p, dim, with_fracs=True)
        if all(abs(f - 0.1) >= 1e-6 for f in fracs):
            return rows
    raise AssertionError("no off-threshold rows")


def check_target(t, rows_list, shapes, params, dim):
    for b, (rows, (H, W), p) in enumerate(zip(rows_list, shapes, params)):
        ref = A.augment_labels(rows, H, W, p, dim)
        n_ref = int((ref.any(1)).sum())
        got = t[b]
        assert np.array_equal(got[:, 0], ref[:, 0].astype(np.float32)), "image %d: kept row set differs" % b
        assert int((got.any(1)).sum()) == n_ref
        assert np.abs(got.astype(np.float64) - ref).max() <= 1e-6
        assert not got[n_ref:].any()


@pytest.mark.parametrize("dim", [(416, 416), (608, 608), (416, 288)])
def test_labels_match_restatement(dim):
    shapes = SHAPES[:6]
    imgs = images(shapes, 4)
    params = np.concatenate([extreme_params(shapes, 0)[:3], aug.sample_params([5, 6, 7], shapes=shapes[3:])])
    # class = the row's index, so that the kept set is compared row by row
    rows_list = []
    for b, ((H, W), p) in enumerate(zip(shapes, params)):
        rows = off_threshold_rows(b + dim[1], 40, H, W, p, dim)
        rows[:, 0] = np.arange(len(rows))
        rows_list.append(rows)
    _, t = run(imgs, rows_list, dim, params)
    assert t.shape == (len(shapes), 90, 5)
    check_target(t, rows_list, shapes, params, dim)
    assert any((t[b].any(1)).sum() < 40 for b in range(len(shapes)))    # some rows were dropped


def test_labels_cap_empty_and_padding():
    shapes = [(480, 640), (480, 640), (300, 300), (300, 300)]
    imgs = images(shapes, 5)
    params = np.tile([0.0, 1.0, 1.0, 0, 0, 0, 0, 0], (4, 1))
    rng = np.random.RandomState(9)
    big = np.zeros((130, 5))
    big[:, 0] = np.arange(130)
    big[:, 1:3] = rng.uniform(0.3, 0.7, (130, 2))
    big[:, 3:5] = rng.uniform(0.05, 0.2, (130, 2))                      # all kept: the first 90 in input order
    small = off_threshold_rows(3, 7, 300, 300, params[2], (416, 416))
    rows_list = [big, np.zeros((0, 5)), small, np.zeros((0, 5))]
    _, t = run(imgs, rows_list, (416, 416), params)
    check_target(t, rows_list, shapes, params, (416, 416))
    assert np.array_equal(t[0, :, 0], np.arange(90, dtype=np.float32))
    assert not t[1].any() and not t[3].any()
    # the same rows as one zero-padded [B,T,5] tensor, on the host and on the GPU
    T = 130
    pad = np.zeros((4, T, 5))
    for b, r in enumerate(rows_list):
        pad[b, :len(r)] = r
    for lab in (torch.from_numpy(pad), torch.from_numpy(pad).to(DEV)):
        _, t2 = run(imgs, lab, (416, 416), params)
        assert np.array_equal(t2, t)
    # no labels at all
    _, t3 = run(imgs, None, (416, 416), params)
    assert not t3.any()


def test_training_step_on_the_output():
    C = 3
    shapes = [(120, 160), (96, 96)]
    imgs = images(shapes, 6)
    params = aug.sample_params([1, 2], shapes=shapes)
    rows = []
    for b, (H, W) in enumerate(shapes):
        r = off_threshold_rows(b + 11, 5, H, W, params[b], (96, 96), C)
        r[:, 3:5] = np.clip(r[:, 3:5], 0.2, 0.6)
        rows.append(r)
    x, target = aug.augment_batch(imgs, rows, (96, 96), params)
    net = YoloNet((96, 96), numClass=C)
    WeightManager(net).load_stream(trained_like_stream(C))
    net = net.to(DEV).train()
    net.backprop = True
    loss = net(x, target)
    loss.backward()
    assert torch.isfinite(loss).item()
    for name, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all().item(), name


def test_deterministic():
    imgs = images(SHAPES, 7)
    params = aug.sample_params(np.arange(len(SHAPES)) * 31, shapes=SHAPES)
    rows = [label_rows(np.random.RandomState(b), 20) for b in range(len(SHAPES))]
    x1, t1 = aug.augment_batch(imgs, rows, (416, 416), params)
    x2, t2 = aug.augment_batch(imgs, rows, (416, 416), params)
    torch.cuda.synchronize()
    assert torch.equal(x1, x2) and torch.equal(t1, t2)
    assert x1.view(torch.int32).equal(x2.view(torch.int32)) and t1.view(torch.int32).equal(t2.view(torch.int32))


# ---- the C-ABI: bounds and error codes ----------------------------------------------------------------------------------------
GUARD = 4096


class Packed:
    """Sources, offsets, hw and params on the device, as augment_batch lays them out."""

    def __init__(self, imgs, params):
        self.B = len(imgs)
        offs, pos = [], 0
        for im in imgs:
            offs.append(pos)
            pos += (im.size + 255) // 256 * 256
        self.src_bytes = pos
        flat = np.zeros(pos, dtype=np.uint8)
        for o, im in zip(offs, imgs):
            flat[o:o + im.size] = im.reshape(-1)
        self.src = torch.from_numpy(flat).to(DEV)
        self.offsets = torch.tensor(offs, dtype=torch.int64, device=DEV)
        self.hw = torch.tensor([im.shape[:2] for im in imgs], dtype=torch.int32, device=DEV)
        self.params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float64)).to(DEV)


def guarded(n, dtype, fill):
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def test_no_byte_outside_outputs_and_workspace_changes():
    imgs = images(SHAPES, 8)
    params = extreme_params(SHAPES, 3)
    pk = Packed(imgs, params)
    lib = _ffi.lib()
    OH, OW, B = 288, 416, pk.B
    xbuf, x = guarded(B * 3 * OH * OW, torch.float32, -7.0)
    wbytes = lib.yv3_augment_workspace_bytes(pk.src_bytes)
    assert wbytes == pk.src_bytes
    wbuf, ws = guarded(wbytes, torch.uint8, 0xA5)
    sbuf, st = guarded(2 * B, torch.int32, 12345)
    rows = [label_rows(np.random.RandomState(b), 30) for b in range(B)]
    lab = torch.from_numpy(np.stack(rows)).to(DEV)
    tbuf, tg = guarded(B * 90 * 5, torch.float32, -9.0)
    s = _ffi.stream_ptr()
    _ffi.check(lib.yv3_augment_images(pk.src.data_ptr(), pk.src_bytes, pk.offsets.data_ptr(), pk.hw.data_ptr(), pk.params.data_ptr(), B,
                                      x.data_ptr(), OH, OW, ws.data_ptr(), wbytes, st.data_ptr(), s))
    _ffi.check(lib.yv3_augment_labels(lab.data_ptr(), B, 30, pk.hw.data_ptr(), pk.params.data_ptr(), tg.data_ptr(), 90, OH, OW,
                                      st.data_ptr() + 4 * B, s))
    torch.cuda.synchronize()
    for buf, fill in ((xbuf, -7.0), (wbuf, 0xA5), (sbuf, 12345), (tbuf, -9.0)):
        assert (buf[:GUARD] == fill).all().item() and (buf[-GUARD:] == fill).all().item()
    assert (st == 0).all().item()
    assert not (x == -7.0).any().item() and not (tg == -9.0).any().item()    # every output element written
    ref = np.stack([A.augment_image(im, p, (OW, OH)) for im, p in zip(imgs, params)])
    assert np.array_equal(x.view(B, 3, OH, OW).cpu().numpy(), ref)


def test_error_codes():
    imgs = images([(20, 30), (40, 10)], 9)
    good = np.array([[0, 1, 1, 0, 0, 0, 0, 0]] * 2, dtype=np.float64)
    pk = Packed(imgs, good)
    lib = _ffi.lib()
    x = torch.empty((2, 3, 64, 64), device=DEV)
    ws = torch.empty(pk.src_bytes, dtype=torch.uint8, device=DEV)
    st = torch.empty(2, dtype=torch.int32, device=DEV)
    tg = torch.empty((2, 90, 5), device=DEV)
    s = _ffi.stream_ptr()

    def images_call(**kw):
        a = dict(src=pk.src.data_ptr(), src_bytes=pk.src_bytes, off=pk.offsets.data_ptr(), hw=pk.hw.data_ptr(),
                 params=pk.params.data_ptr(), B=2, out=x.data_ptr(), oh=64, ow=64, ws=ws.data_ptr(), wsb=ws.numel(),
                 st=st.data_ptr())
        a.update(kw)
        return lib.yv3_augment_images(a["src"], a["src_bytes"], a["off"], a["hw"], a["params"], a["B"], a["out"], a["oh"], a["ow"],
                                      a["ws"], a["wsb"], a["st"], s)

    assert images_call() == 0
    for kw in (dict(src=None), dict(off=None), dict(hw=None), dict(params=None), dict(out=None), dict(ws=None), dict(st=None),
               dict(B=0), dict(B=-1), dict(oh=0), dict(ow=-5), dict(src_bytes=0)):
        assert images_call(**kw) == _ffi.EINVAL, kw
    assert images_call(wsb=ws.numel() - 1) == _ffi.EWORKSPACE
    assert lib.yv3_augment_workspace_bytes(0) == 0

    def labels_call(lab, T, B=2, mr=90, target=None, status=None):
        return lib.yv3_augment_labels(lab, B, T, pk.hw.data_ptr(), pk.params.data_ptr(), target if target is not None else tg.data_ptr(),
                                      mr, 64, 64, status if status is not None else st.data_ptr(), s)

    lab = torch.zeros((2, 3, 5), dtype=torch.float64, device=DEV)
    assert labels_call(lab.data_ptr(), 3) == 0 and labels_call(None, 0) == 0
    assert labels_call(None, 3) == _ffi.EINVAL and labels_call(lab.data_ptr(), -1) == _ffi.EINVAL
    assert labels_call(lab.data_ptr(), 3, B=0) == _ffi.EINVAL and labels_call(lab.data_ptr(), 3, mr=0) == _ffi.EINVAL
    assert lib.yv3_augment_labels(lab.data_ptr(), 2, 3, None, pk.params.data_ptr(), tg.data_ptr(), 90, 64, 64, st.data_ptr(), s) == _ffi.EINVAL
    torch.cuda.synchronize()

    # per-image parameters: found on the device, reported in status[b]; the image's outputs are zeros
    bad_rows = [([np.nan, 1, 1, 0, 0, 0, 0, 0], _ffi.EINVAL), ([0, np.inf, 1, 0, 0, 0, 0, 0], _ffi.EINVAL),
                ([0, 1, -1, 0, 0, 0, 0, 0], _ffi.EINVAL), ([0, 1, 1, 0.5, 0, 0, 0, 0], _ffi.EINVAL),
                ([0, 1, 1, 0, 0, 0, 0, 0.5], _ffi.EINVAL), ([0, 1, 1, -20, 0, -20, 0, 0], _ffi.ESHAPE),
                ([0, 1, 1, 0, -15, 0, -15, 0], _ffi.ESHAPE)]
    for row, code in bad_rows:
        p = torch.tensor(np.array([good[0], row], dtype=np.float64), device=DEV)
        x.fill_(-1.0)
        tg.fill_(-1.0)
        assert images_call(params=p.data_ptr()) == 0
        torch.cuda.synchronize()
        assert st.tolist() == [0, code], row
        assert (x[1] == 0).all().item() and (x[0] >= 0).all().item()
        lab = torch.tensor([[[1, 0.5, 0.5, 0.2, 0.2]]] * 2, dtype=torch.float64, device=DEV)
        assert lib.yv3_augment_labels(lab.data_ptr(), 2, 1, pk.hw.data_ptr(), p.data_ptr(), tg.data_ptr(), 90, 64, 64, st.data_ptr(), s) == 0
        torch.cuda.synchronize()
        assert st.tolist() == [0, code] and not tg[1].any().item() and tg[0, 0, 0].item() == 1.0
        # augment_batch refuses the same row on the host, before any launch
        with pytest.raises(_ffi.Yv3Error) as e:
            aug.augment_batch(imgs, None, (64, 64), np.array([good[0], row]))
        assert e.value.code == code
    # a source that does not fit in src_bytes
    bad_off = torch.tensor([0, pk.src_bytes - 10], dtype=torch.int64, device=DEV)
    assert images_call(off=bad_off.data_ptr()) == 0
    torch.cuda.synchronize()
    assert st.tolist() == [0, _ffi.EINVAL]


# ---- loader -------------------------------------------------------------------------------------------------------------------
def test_train_batches_from_a_list_file(tmp_path):
    from PIL import Image
    (tmp_path / "images").mkdir()
    (tmp_path / "labels").mkdir()
    shapes = [(120, 160), (90, 70), (64, 64), (100, 200), (33, 47)]
    imgs = images(shapes, 10)
    paths, rows_list = [], []
    for i, im in enumerate(imgs):
        p = str(tmp_path / "images" / ("img%d.jpg" % i))                 # PNG bytes under the reference's .jpg naming: lossless
        Image.fromarray(im).save(p, format="PNG")
        paths.append(p)
        rows = off_threshold_rows(i, 4, im.shape[0], im.shape[1], [0, 1, 1, 0, 0, 0, 0, 0], (128, 96))
        if i != 2:                                                       # image 2 has no label file
            np.savetxt(str(tmp_path / "labels" / ("img%d.txt" % i)), rows)
            rows_list.append(np.loadtxt(str(tmp_path / "labels" / ("img%d.txt" % i))).reshape(-1, 5))
        else:
            rows_list.append(np.zeros((0, 5)))
    lst = tmp_path / "train.txt"
    lst.write_text("\n".join(paths) + "\n")
    loader = aug.TrainBatches(str(lst), 2, (128, 96), seed=4, jitter=0.2)
    assert len(loader) == 3
    batches = [(x.cpu().numpy(), t.cpu().numpy()) for x, t in loader]
    assert [b[0].shape[0] for b in batches] == [2, 2, 1]
    # the documented streams: RandomState([seed, epoch]) -> permutation, then one seed per image
    rng = np.random.RandomState([4, 0])
    order = rng.permutation(5)
    seeds = rng.randint(0, 2 ** 31 - 1, size=5)
    for k, (x, t) in enumerate(batches):
        idx = order[2 * k:2 * k + 2]
        params = aug.sample_params(seeds[2 * k:2 * k + len(idx)], shapes=[shapes[j] for j in idx], jitter=0.2)
        for i, j in enumerate(idx):
            assert np.array_equal(x[i], A.augment_image(imgs[j], params[i], (128, 96)))
            ref = A.augment_labels(rows_list[j], shapes[j][0], shapes[j][1], params[i], (128, 96))
            assert np.array_equal(t[i, :, 0], ref[:, 0].astype(np.float32)) and np.abs(t[i] - ref).max() <= 1e-6
    again = [(x.cpu().numpy(), t.cpu().numpy()) for x, t in aug.TrainBatches(str(lst), 2, (128, 96), seed=4, jitter=0.2)]
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(batches, again))
    second_epoch = [x.cpu().numpy() for x, _ in loader]
    assert not all(np.array_equal(a[0], b) for a, b in zip(batches, second_epoch))
