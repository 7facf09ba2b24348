"""The affine augmentation on the GPU (csrc/affine_augment.hip, yolo_v3_amd/affine_augment.py) against the numpy restatement
tests/affine_aug_ref.py: pixels and labels bit for bit, no tolerance and no excluded bytes.

The pixel kernel's tile is 4 rows x 64 pixels (AF_TH x AF_TW), a wave per tile row: 4 x 64 is exactly one tile, 5 x 65 one tile
plus one pixel in each direction, 97 x 130 exceeds it in both dimensions by a non-multiple.  The label kernel strides an image's
rows over the 64 lanes of one wave: T = 64 fills the wave once, T = 65 starts the second round.
"""
import math

import numpy as np
import pytest
import torch

from tests import affine_aug_ref as R
from yolo_v3_amd import _ffi, evaluate
from yolo_v3_amd import affine_augment as affine
from yolo_v3_amd import augment as aug

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
SIZES = [(1, 1), (1, 7), (7, 1), (4, 64), (5, 65), (33, 65), (97, 130)]


def image(h, w, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 97) % 256], -1)
    return np.clip(base + rng.randint(-60, 61, (h, w, 3)), 0, 255).astype(np.uint8)


def program(h, w, active=1, **kw):
    fwd, inv = affine.affine_matrices(h, w, **kw)
    return {"active": active, "shape": (h, w), "fwd": fwd, "inv": inv}


def dev_i64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def upload(packed):
    return torch.from_numpy(packed.view(np.uint8).reshape(-1).copy()).to(DEV)


def run_raw(imgs, sources, packed, src_off, src_total, out_off, out_total, fill=0x5A, calls=1, out_bytes=None):
    """yv3_affine_augment: image b is `imgs[sources[b]]`, read at `src_off[sources[b]]` of an allocation of `src_total` random
    bytes and written at `out_off[b]` of `out_total` bytes between two guards.  `out_bytes`: the length passed to the library
    (by default `out_total`).  Returns (outputs, status, the raw `out` bytes)."""
    B = len(sources)
    arena_np = np.random.RandomState(5).randint(0, 256, src_total).astype(np.uint8)
    for o, im in zip(src_off, imgs):
        arena_np[o:o + im.size] = im.reshape(-1)
    arena = torch.from_numpy(arena_np).to(DEV)
    hw = torch.tensor([imgs[j].shape[:2] for j in sources], dtype=torch.int32, device=DEV)
    prog = upload(packed)
    soff, ooff = dev_i64([src_off[j] for j in sources]), dev_i64(out_off)
    lib = _ffi.lib()
    results = []
    for _ in range(calls):
        obuf = torch.full((GUARD + out_total + GUARD,), fill, dtype=torch.uint8, device=DEV)
        out = obuf[GUARD:GUARD + out_total]
        st = torch.full((B + 2,), 12345, dtype=torch.int32, device=DEV)
        _ffi.check(lib.yv3_affine_augment(arena.data_ptr(), arena.numel(), soff.data_ptr(), hw.data_ptr(), prog.data_ptr(), B,
                                          out.data_ptr(), out_total if out_bytes is None else out_bytes, ooff.data_ptr(),
                                          st[1:].data_ptr(), _ffi.stream_ptr()), "yv3_affine_augment")
        torch.cuda.synchronize()
        assert (obuf[:GUARD] == fill).all().item() and (obuf[-GUARD:] == fill).all().item()
        assert st[0].item() == 12345 and st[-1].item() == 12345
        assert np.array_equal(arena.cpu().numpy(), arena_np)                       # the sources are only read
        raw = out.cpu().numpy()
        status = st[1:-1].tolist()
        gaps = np.ones(out_total, dtype=bool)
        for o, j, code in zip(out_off, sources, status):
            if o >= 0 and o + imgs[j].size <= (out_total if out_bytes is None else out_bytes):
                gaps[o:o + imgs[j].size] = False
        assert (raw[gaps] == fill).all()                                           # nothing written between or past the images
        results.append(([raw[o:o + imgs[j].size].reshape(imgs[j].shape) for o, j in zip(out_off, sources)], status, raw))
    for r in results[1:]:
        assert np.array_equal(r[2], results[0][2])                                 # identical calls, identical bits
    return results[0]


def odd_layout(sizes, start, gap):
    offs, pos = [], start
    for n in sizes:
        offs.append(pos)
        pos = (pos + n + gap) | 1
    return offs, pos


def eight():
    """Eight images of the seven sizes: 33 x 65 is used twice, under different programs; 1 x 7 is inactive."""
    imgs = [image(h, w, 40 + i) for i, (h, w) in enumerate(SIZES)]
    sources = [0, 1, 2, 3, 4, 5, 6, 5]
    kinds = [dict(theta=math.radians(20), scale=1.3),
             dict(theta=math.radians(10), tx=0.1),
             dict(theta=math.radians(-45), scale=0.5, shear=math.radians(20)),
             dict(theta=math.radians(8), scale=1.1, shear=math.radians(-5), tx=0.05, ty=-0.1),
             dict(theta=math.radians(-30), scale=0.8, tx=-0.2, ty=0.3),
             dict(theta=math.radians(45), scale=2.0, shear=math.radians(-20), tx=0.1),
             dict(theta=math.radians(-17), scale=0.7, shear=math.radians(12), tx=0.25, ty=-0.2),
             dict()]                                                               # the identity, active
    programs = [program(*imgs[j].shape[:2], active=0 if j == 1 else 1, **kw) for j, kw in zip(sources, kinds)]
    return imgs, sources, programs


def test_pixels_packed_and_gathered_bit_for_bit():
    imgs, sources, programs = eight()
    batch = [imgs[j] for j in sources]
    affine.check_affine_programs(programs, [im.shape[:2] for im in batch])
    ref = [R.warp_ref(im, p) for im, p in zip(batch, programs)]
    assert np.array_equal(ref[1], imgs[1]) and np.array_equal(ref[7], imgs[5]) and not np.array_equal(ref[5], ref[7])
    assert all((r == 128).any() and (r != 128).any() for r in ref[3:7])            # the pad and the image both occur
    packed = affine.pack_programs(programs)
    # packed: sources and outputs back to back, at odd byte offsets
    src_off, src_total = odd_layout([im.size for im in imgs], 1, 0)
    out_off, out_total = odd_layout([im.size for im in batch], 3, 0)
    assert all(o % 2 == 1 for o in src_off + out_off)
    got, status, _ = run_raw(imgs, sources, packed, src_off, src_total, out_off, out_total, calls=2)
    assert status == [0] * 8
    for b, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g, r), "image %d %s: %d bytes differ" % (b, r.shape, int((g != r).sum()))
    # gathered from a larger allocation, guard bytes before, between and after (run_raw checks the allocation and the gaps of `out`)
    src_off, src_total = odd_layout([im.size for im in imgs], 777, 300)
    out_off, out_total = odd_layout([im.size for im in batch], 513, 200)
    far, status, _ = run_raw(imgs, sources, packed, src_off, src_total + 999, out_off, out_total + 500, fill=0xC3)
    assert status == [0] * 8
    for g, f in zip(got, far):
        assert np.array_equal(g, f)


def label_rows(rng, T, n):
    """[T,5]: n random rows (some partly or wholly outside, some empty), then zero padding."""
    rows = np.zeros((T, 5))
    n = min(n, T)
    rows[:n, 0] = rng.randint(0, 80, n)
    rows[:n, 1:3] = rng.uniform(-0.2, 1.2, (n, 2))
    rows[:n, 3:5] = rng.uniform(0.02, 0.6, (n, 2))
    rows[:n:7, 3] = 0.0                                                            # w == 0: dropped by label_np_to_bbs
    rows[3:n:11, 4] = -0.1
    return rows


@pytest.mark.parametrize("T", [0, 1, 64, 65])
def test_labels_bit_for_bit(T):
    rng = np.random.RandomState(T)
    shapes = [(48, 64), (97, 130), (1, 7), (33, 65), (480, 640)]
    programs = [program(48, 64, theta=math.radians(15), scale=1.2, tx=0.1),
                program(97, 130, active=0, theta=0.5),
                program(1, 7),
                program(33, 65, theta=math.radians(-40), scale=0.6, shear=math.radians(15), tx=-0.3, ty=0.2),
                program(480, 640, theta=math.radians(90))]
    B = len(shapes)
    labels = np.stack([label_rows(rng, T, n) for n in (T, T, T // 2, max(T - 3, 0), T)]) if T else np.zeros((B, 0, 5))
    ref = np.stack([R.labels_ref(l, h, w, p) for l, (h, w), p in zip(labels, shapes, programs)])
    if T >= 64:
        kept = ref[[0, 3, 4]][..., 3] > 0
        assert kept.any() and not kept.all()                                       # rows that stay and rows that drop
        assert np.array_equal(ref[1].view(np.int64), labels[1].view(np.int64))     # inactive: passed through
    lib = _ffi.lib()
    hw = torch.tensor(shapes, dtype=torch.int32, device=DEV)
    prog = upload(affine.pack_programs(programs))
    for alias in (False, True):
        buf = torch.full((16 + B * T * 5 + 16,), 7.5, dtype=torch.float64, device=DEV)
        lab = torch.from_numpy(labels).to(DEV)
        if alias:
            buf[16:16 + B * T * 5].copy_(lab.reshape(-1))
            lab = buf[16:16 + B * T * 5]
        out = buf[16:16 + B * T * 5]
        st = torch.full((B + 2,), 12345, dtype=torch.int32, device=DEV)
        _ffi.check(lib.yv3_affine_labels(lab.data_ptr() if T else None, B, T, hw.data_ptr(), prog.data_ptr(),
                                         out.data_ptr() if T else None, st[1:].data_ptr(), _ffi.stream_ptr()), "yv3_affine_labels")
        torch.cuda.synchronize()
        assert st.tolist() == [12345] + [0] * B + [12345]
        assert (buf[:16] == 7.5).all().item() and (buf[-16:] == 7.5).all().item()
        got = out.cpu().numpy().reshape(B, T, 5)
        assert np.array_equal(got.view(np.int64), ref.view(np.int64)), (T, alias, int((got != ref).sum()))


def test_a_malformed_image_is_reported_for_it_only():
    """Every case is caught by a check before any access: a NaN coefficient, active = 2, an out range past out_bytes."""
    imgs = [image(33, 65, 70 + i) for i in range(5)]
    sources = [0, 1, 2, 3, 4]
    kw = dict(theta=math.radians(12), scale=1.1, tx=0.05)
    programs = [program(33, 65, **kw) for _ in range(5)]
    packed = affine.pack_programs(programs)
    packed["inv"][1][4] = np.nan
    packed["active"][2] = 2
    n = imgs[0].size
    src_off, src_total = odd_layout([n] * 5, 1, 10)
    out_off = [1, n + 3, 2 * n + 5, 4 * n + 7, 3 * n + 7]                           # image 3 would end 7 bytes past the 5 n bytes passed
    got, status, raw = run_raw(imgs, sources, packed, src_off, src_total, out_off, 5 * n + 64, out_bytes=5 * n)
    assert status == [0, _ffi.EINVAL, _ffi.EINVAL, _ffi.EINVAL, 0]
    good = R.warp_ref(imgs[0], programs[0])
    assert np.array_equal(got[0], good) and np.array_equal(got[4], R.warp_ref(imgs[4], programs[4]))
    assert np.array_equal(got[1], imgs[1]) and np.array_equal(got[2], imgs[2])     # copied through
    assert (raw[4 * n + 7:] == 0x5A).all()                                         # nothing written for image 3, inside or past out_bytes

    # the labels of the same programs: passed through for the two malformed ones
    rng = np.random.RandomState(3)
    labels = np.stack([label_rows(rng, 9, 8) for _ in range(5)])
    lab, out = torch.from_numpy(labels).to(DEV), torch.full((5, 9, 5), 7.5, dtype=torch.float64, device=DEV)
    hw = torch.tensor([[33, 65]] * 5, dtype=torch.int32, device=DEV)
    prog = upload(packed)
    st = torch.full((5,), 12345, dtype=torch.int32, device=DEV)
    lib = _ffi.lib()
    args = [lab.data_ptr(), 5, 9, hw.data_ptr(), prog.data_ptr(), out.data_ptr(), st.data_ptr(), _ffi.stream_ptr()]
    assert lib.yv3_affine_labels(*args) == 0
    torch.cuda.synchronize()
    assert st.tolist() == [0, _ffi.EINVAL, _ffi.EINVAL, 0, 0]
    got_l = out.cpu().numpy()
    for b in range(5):
        want = labels[b] if b in (1, 2) else R.labels_ref(labels[b], 33, 65, programs[b])
        assert np.array_equal(got_l[b].view(np.int64), want.view(np.int64)), b
    assert not np.array_equal(got_l[0], labels[0])

    # H or W <= 0: EINVAL, rows passed through
    hw0 = torch.tensor([[33, 65], [0, 65], [33, -1], [33, 65], [33, 65]], dtype=torch.int32, device=DEV)
    clean = upload(affine.pack_programs(programs))
    out.fill_(7.5)
    assert lib.yv3_affine_labels(lab.data_ptr(), 5, 9, hw0.data_ptr(), clean.data_ptr(), out.data_ptr(), st.data_ptr(),
                                 _ffi.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert st.tolist() == [0, _ffi.EINVAL, _ffi.EINVAL, 0, 0]
    assert np.array_equal(out[1:3].cpu().numpy().view(np.int64), labels[1:3].view(np.int64))

    # host arguments: refused before any launch (status and outputs keep their fill)
    out.fill_(7.5)
    st.fill_(12345)
    for i in (0, 3, 4, 5, 6):                                                       # each pointer as NULL
        bad = list(args)
        bad[i] = None
        assert lib.yv3_affine_labels(*bad) == _ffi.EINVAL
    for i, v in ((1, 0), (1, -1), (2, -1)):
        bad = list(args)
        bad[i] = v
        assert lib.yv3_affine_labels(*bad) == _ffi.EINVAL
    src = torch.from_numpy(imgs[0].reshape(-1).copy()).to(DEV)
    res = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    zero, hw1 = dev_i64([0]), torch.tensor([[33, 65]], dtype=torch.int32, device=DEV)
    pargs = [src.data_ptr(), n, zero.data_ptr(), hw1.data_ptr(), prog.data_ptr(), 1, res.data_ptr(), n, zero.data_ptr(), st.data_ptr(),
             _ffi.stream_ptr()]
    for i in (0, 2, 3, 4, 6, 8, 9):
        bad = list(pargs)
        bad[i] = None
        assert lib.yv3_affine_augment(*bad) == _ffi.EINVAL
    for i, v in ((1, 0), (1, -5), (5, 0), (5, -1), (5, 65536), (7, 0), (7, -1)):
        bad = list(pargs)
        bad[i] = v
        assert lib.yv3_affine_augment(*bad) == _ffi.EINVAL
    torch.cuda.synchronize()
    assert st.tolist() == [12345] * 5 and (res == 0x5A).all().item() and (out == 7.5).all().item()
    # a source that ends one byte past its allocation, and a negative offset: refused on the device, not read
    for off in (1, -1):
        soff = dev_i64([off])
        assert lib.yv3_affine_augment(*(pargs[:2] + [soff.data_ptr()] + pargs[3:])) == 0
        torch.cuda.synchronize()
        assert st[0].item() == _ffi.EINVAL and (res == 0x5A).all().item()
    with pytest.raises(_ffi.Yv3Error) as e:                                        # the Python entrance checks on the host first
        affine.affine_augment_batch([imgs[0]], None, [dict(programs[0], active=2)])
    assert e.value.code == _ffi.EINVAL


def test_affine_augment_batch_entrances_and_what_it_feeds():
    shapes = [(48, 64), (64, 48), (33, 65), (5, 65), (97, 130), (48, 64), (40, 56), (1, 7)]
    imgs = [image(h, w, 90 + i) for i, (h, w) in enumerate(shapes)]
    rng = np.random.RandomState(9)
    labels = [label_rows(rng, n, n) for n in (3, 0, 5, 1, 2, 4, 3, 1)]
    programs = affine.sample_affine(range(8), shapes, rotate=(-30, 30), scale=(0.7, 1.4), p=0.75)
    assert 0 < sum(p["active"] for p in programs) < 8
    ref_i, ref_l = R.affine_ref(imgs, labels, programs)
    arena = torch.empty(sum(im.size + 256 for im in imgs), dtype=torch.uint8, device=DEV)
    views, pos = [], 0
    for im in imgs:
        v = arena[pos:pos + im.size].view(im.shape)
        v.copy_(torch.from_numpy(im))
        views.append(v)
        pos = (pos + im.size + 255) // 256 * 256
    pixel_bytes = sum(im.size for im in imgs)
    padded = torch.zeros((8, 5, 5), dtype=torch.float64)
    for b, l in enumerate(labels):
        padded[b, :len(l)] = torch.from_numpy(l)
    for what, lab in ((imgs, labels), (views, labels), ([torch.from_numpy(im).to(DEV) for im in imgs], padded), (views, padded.to(DEV))):
        before = aug.counters["upload_bytes"]
        out, lout = affine.affine_augment_batch(what, lab, programs)
        uploaded = aug.counters["upload_bytes"] - before
        assert (uploaded < pixel_bytes) == (what is not imgs)                      # only host images are uploaded; views are gathered
        assert all(o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() for o in out)
        assert len({o.untyped_storage().data_ptr() for o in out}) == 1             # what the next stages' gather path asks for
        assert lout.is_cuda and lout.dtype == torch.float64 and tuple(lout.shape) == (8, 5, 5)
        for o, r in zip(out, ref_i):
            assert np.array_equal(o.cpu().numpy(), r)
        got_l = lout.cpu().numpy()
        for b, r in enumerate(ref_l):
            assert np.array_equal(got_l[b, :len(r)].view(np.int64), r.view(np.int64)) and not got_l[b, len(r):].any()
    assert all(np.array_equal(v.cpu().numpy(), im) for v, im in zip(views, imgs))
    assert np.array_equal(padded[0, :3].numpy(), labels[0])                        # a label tensor passed in is not written
    out_none, l_none = affine.affine_augment_batch(views, None, programs)
    assert tuple(l_none.shape) == (8, 0, 5) and all(np.array_equal(o.cpu().numpy(), r) for o, r in zip(out_none, ref_i))

    # the outputs feed the next stages without a copy of the pixels: both take their gather path
    extras = aug.sample_extra(range(8), shapes)
    params = aug.sample_params(range(8), shapes=shapes, jitter=0.2)
    before = aug.counters["upload_bytes"]
    blurred = aug.extra_augment_batch(out, extras)
    x, target = aug.augment_batch(blurred, lout, (96, 96), params)
    assert aug.counters["upload_bytes"] - before < pixel_bytes // 4
    x0, target0 = aug.augment_batch(aug.extra_augment_batch(ref_i, extras), ref_l, (96, 96), params)
    assert torch.equal(x, x0) and torch.equal(target, target0) and target.any().item()


# ---- the loader ---------------------------------------------------------------------------------------------------------------------
LOADER_SHAPES = [(48, 64), (64, 48), (48, 64), (40, 56), (33, 65), (48, 64), (56, 40), (48, 64)]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("affine_loader")
    (root / "images").mkdir()
    (root / "labels").mkdir()
    rng = np.random.RandomState(31)
    paths = []
    for i, (h, w) in enumerate(LOADER_SHAPES):
        p = str(root / "images" / ("img%d.jpg" % i))
        Image.fromarray(image(h, w, 100 + i)).save(p, format="JPEG", quality=90)
        paths.append(p)
        rows = np.column_stack([rng.randint(0, 3, 3), rng.uniform(0.1, 0.9, (3, 2)), rng.uniform(0.1, 0.5, (3, 2))])
        np.savetxt(str(root / "labels" / ("img%d.txt" % i)), rows)
    lst = root / "train.txt"
    lst.write_text("\n".join(paths) + "\n")
    return str(lst), paths


def epochs(loader, n):
    return [[(x.cpu().numpy(), t.cpu().numpy()) for x, t in loader] for _ in range(n)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.int32), x0.view(np.int32)) and np.array_equal(t.view(np.int32), t0.view(np.int32))
                                    for (x, t), (x0, t0) in zip(a, b))


def restated(paths, seed, epoch, with_extra):
    """An epoch's batches from the host reference: augment_batch on tests/affine_aug_ref.py's warped images and labels."""
    order, seeds, _ = aug.epoch_schedule(seed, epoch, len(paths), 4)
    out = []
    for k in range(2):
        idx = [int(j) for j in order[4 * k:4 * k + 4]]
        srcs = [evaluate.read_image_rgb(paths[j]) for j in idx]
        shapes = [s.shape[:2] for s in srcs]
        programs = affine.sample_affine(seeds[4 * k:4 * k + 4], shapes)
        params = aug.sample_params(seeds[4 * k:4 * k + 4], shapes=shapes, jitter=0.2)
        images, labels = R.affine_ref(srcs, [aug.read_labels(aug.label_path(paths[j])) for j in idx], programs)
        if with_extra:
            images = aug.extra_augment_batch(images, aug.sample_extra(seeds[4 * k:4 * k + 4], shapes))
        x, t = aug.augment_batch(images, labels, (96, 96), params)
        out.append((x.cpu().numpy(), t.cpu().numpy()))
    return out, sum(p["active"] for k in range(2) for p in affine.sample_affine(seeds[4 * k:4 * k + 4], [(48, 64)] * 4))


def test_train_batches_with_affine(listing):
    lst, paths = listing
    kw = dict(seed=4, jitter=0.2)
    base = epochs(aug.TrainBatches(lst, 4, (96, 96), affine=True, **kw), 2)
    assert [len(e) for e in base] == [2, 2]
    for e in range(2):
        want, n_active = restated(paths, 4, e, False)
        assert 0 < n_active < 8                                                    # some images are warped, some are not
        assert same(base[e], want), e
    assert all(t.any() for _, t in base[0])                                        # label rows arrive
    # the same bits with decode threads, with the arena (second epoch: every source resident, gathered in place), with GPU decode
    full = aug.TrainBatches(lst, 4, (96, 96), **kw).decoded_bytes()
    for conf in (dict(workers=2), dict(cache_bytes=full), dict(decode="gpu", cache_bytes=full)):
        loader = aug.TrainBatches(lst, 4, (96, 96), affine=True, **kw, **conf)
        got = epochs(loader, 2)
        assert same(got[0], base[0]) and same(got[1], base[1]), conf
        if "cache_bytes" in conf:
            assert loader.resident_images() == len(paths)
    # with the extras as well: affine, then extras, then augment_batch
    both = epochs(aug.TrainBatches(lst, 4, (96, 96), affine=True, extra=True, **kw), 1)
    assert same(both[0], restated(paths, 4, 0, True)[0]) and not same(both[0], base[0])
    # across a resume
    loader = aug.TrainBatches(lst, 4, (96, 96), affine=True, **kw)
    it = iter(loader)
    next(it)
    state = loader.state_dict()
    assert state["config"]["affine"] is True and state["batch"] == 1
    it.close()
    fresh = aug.TrainBatches(lst, 4, (96, 96), affine=True, **kw)
    fresh.load_state_dict(state)
    assert same(epochs(fresh, 1)[0], base[0][1:])
    with pytest.raises(ValueError):
        aug.TrainBatches(lst, 4, (96, 96), **kw).load_state_dict(state)            # a loader without the switch refuses the state
    # off: the loader is what it was, its state dict carries no new key, and a state from a loader without the switch loads
    plain, off = aug.TrainBatches(lst, 4, (96, 96), **kw), aug.TrainBatches(lst, 4, (96, 96), affine=None, **kw)
    assert "affine" not in off.state_dict()["config"] and off.state_dict() == plain.state_dict()
    a, b = epochs(plain, 1)[0], epochs(off, 1)[0]
    assert same(a, b) and not same(a, base[0])
    off.load_state_dict(plain.state_dict())
    # a dict of sample_affine's arguments: p = 0 fires for no image, and the batches are the plain loader's
    never = epochs(aug.TrainBatches(lst, 4, (96, 96), affine=dict(p=0.0), **kw), 1)[0]
    assert same(never, a)
