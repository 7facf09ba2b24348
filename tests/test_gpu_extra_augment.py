"""The reference's ExtraAugmentations on the GPU (csrc/extra_augment.hip, yolo_v3_amd/extra_augment.py) against the numpy
restatement tests/extra_aug_ref.py: bit for bit, with NOISE as the one exception (below).

The kernel's tile is 32 rows x 64 pixels (EX_TH x EX_TW): the 70 x 130 image exceeds it in both dimensions by a non-multiple, the
others are smaller than one tile and some smaller than every halo (the borders' periodic case).

NOISE: the device's float64 log and cos may differ from numpy's in the last place, so a byte may differ by 1 where the
restatement's value before clip and truncation lies within 1e-9 of an integer (`extra_aug_ref.noise_mask`); outside that mask
the comparison is exact, and the mask may cover at most 1 in 10^5 of the compared bytes.
"""
import numpy as np
import pytest
import torch

from tests import extra_aug_ref as R
from yolo_v3_amd import _ffi, evaluate
from yolo_v3_amd import augment as aug
from yolo_v3_amd import extra_augment as extra

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
SIZES = [(1, 1), (1, 7), (5, 3), (13, 9), (33, 47), (70, 130)]
KEY = 0x0123456789ABCDEF


def image(h, w, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 97) % 256], -1)
    return np.clip(base + rng.randint(-60, 61, (h, w, 3)), 0, 255).astype(np.uint8)


def ramp():
    return np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (2, 256, 3)))


def dev_i64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def guarded(n, fill):
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def run_raw(imgs, packed, fill=0x5A, calls=1):
    """yv3_extra_augment on sources gathered from inside a larger allocation (odd byte offsets, noise in between), outputs at odd
    multiples of 256 with guard bytes around `out` and the workspace.  Returns (outputs, status, the raw `out` bytes)."""
    B = len(imgs)
    src_off, pos = [], 7
    for im in imgs:
        src_off.append(pos)
        pos = (pos + im.size + 100) | 1
    arena_np = np.random.RandomState(5).randint(0, 256, pos + 333).astype(np.uint8)
    for o, im in zip(src_off, imgs):
        arena_np[o:o + im.size] = im.reshape(-1)
    out_off, pos = [], 256
    for im in imgs:
        out_off.append(pos)
        pos = ((pos + im.size + 255) // 256 * 256) | 256                           # the next odd multiple of 256
    assert all(o % 512 == 256 for o in out_off)
    out_bytes = pos
    arena = torch.from_numpy(arena_np).to(DEV)
    hw = torch.tensor([im.shape[:2] for im in imgs], dtype=torch.int32, device=DEV)
    prog = torch.from_numpy(packed.view(np.uint8).reshape(-1).copy()).to(DEV)
    soff, ooff = dev_i64(src_off), dev_i64(out_off)
    lib = _ffi.lib()
    assert lib.yv3_extra_augment_workspace_bytes(out_bytes) == out_bytes
    results = []
    for _ in range(calls):
        obuf, out = guarded(out_bytes, fill)
        wbuf, ws = guarded(out_bytes, 0xA5)
        st = torch.full((B + 2,), 12345, dtype=torch.int32, device=DEV)
        _ffi.check(lib.yv3_extra_augment(arena.data_ptr(), arena.numel(), soff.data_ptr(), hw.data_ptr(), prog.data_ptr(), B,
                                         out.data_ptr(), out_bytes, ooff.data_ptr(), ws.data_ptr(), out_bytes,
                                         st[1:].data_ptr(), _ffi.stream_ptr()), "yv3_extra_augment")
        torch.cuda.synchronize()
        for buf, f in ((obuf, fill), (wbuf, 0xA5)):
            assert (buf[:GUARD] == f).all().item() and (buf[-GUARD:] == f).all().item()
        assert st[0].item() == 12345 and st[-1].item() == 12345
        assert np.array_equal(arena.cpu().numpy(), arena_np)                       # the sources are only read
        raw = out.cpu().numpy()
        gaps = np.ones(out_bytes, dtype=bool)
        for o, im in zip(out_off, imgs):
            gaps[o:o + im.size] = False
        assert (raw[gaps] == fill).all()                                           # nothing written between the images
        results.append(([raw[o:o + im.size].reshape(im.shape) for o, im in zip(out_off, imgs)], st[1:-1].tolist(), raw))
    for r in results[1:]:
        assert np.array_equal(r[2], results[0][2])                                 # identical calls, identical bits
    return results[0]


def compare(got, imgs, programs):
    """Exact outside the NOISE mask, at most 1 inside it, the mask at most 1e-5 of the bytes.  Returns the mask's count."""
    ref = R.extra_ref(imgs, programs)
    total = masked = 0
    for b, (g, r, im, prog) in enumerate(zip(got, ref, imgs, programs)):
        mask = R.program_noise_mask(im, prog)
        diff = np.abs(g.astype(np.int32) - r.astype(np.int32))
        assert not diff[~mask].any(), "image %d %s program %r: %d bytes differ, max %d" % (
            b, im.shape, prog, int((diff[~mask] != 0).sum()), int(diff.max()))
        assert diff[mask].max(initial=0) <= 1
        total += mask.size
        masked += int(mask.sum())
    assert masked * 10 ** 5 <= total
    return masked


SINGLE = [[("GAUSS", 0.05)], [("GAUSS", 3.0)], [("GAUSS", 0.7)], [("AVERAGE", 2)], [("AVERAGE", 7)], [("MEDIAN", 3)], [("MEDIAN", 11)],
          [("SHARPEN", 0.0, 0.75)], [("SHARPEN", 0.5, 1.5)], [("SHARPEN", 0.0, 1.5)], [("SHARPEN", 0.5, 0.75)],
          [("ADD", 5, 5, 5)], [("ADD", -5, -5, -5)], [("ADD", -5, 0, 5)], [("MUL", 0.8, 0.8, 0.8)], [("MUL", 1.2, 1.2, 1.2)],
          [("MUL", 0.8, 1.0, 1.2)], [("CONTRAST", 0.5, 0.5, 0.5)], [("CONTRAST", 2.0, 2.0, 2.0)], [("CONTRAST", 0.5, 1.0, 2.0)],
          [("NOISE", 0.0, False, KEY)], [("NOISE", 0.0, True, KEY)], [("NOISE", 12.75, False, KEY)], [("NOISE", 12.75, True, KEY)],
          []]


def test_each_operation_alone_at_both_ends_of_its_range():
    srcs = [image(h, w, 40 + i) for i, (h, w) in enumerate(SIZES)] + [ramp()]
    imgs, programs = [], []
    for prog in SINGLE:                                                            # every size under every program, in one batch
        for im in srcs:
            imgs.append(im)
            programs.append(prog)
    extra.check_programs(programs, [im.shape[:2] for im in imgs])
    got, status, _ = run_raw(imgs, extra.pack_programs(programs))
    assert status == [0] * len(imgs)
    masked = compare(got, imgs, programs)
    assert masked == 0                                                             # observed on the CPU: 0 of the 67 818 bytes under scale 12.75
    n = len(srcs)
    for i in (0, 7, 9, 20, 21, 24):                                                # sigma 0.05 (skipped), alpha 0, scale 0, no steps
        for g, im in zip(got[i * n:(i + 1) * n], srcs):
            assert np.array_equal(g, im), SINGLE[i]
    lo, hi = got[12 * n + n - 1], got[11 * n + n - 1]                              # add -5 / +5 on the ramp: saturation at both ends
    assert lo[0, :6, 0].tolist() == [0] * 6 and hi[0, -6:, 0].tolist() == [255] * 6


def test_constant_images_through_gauss_truncate_like_scipy():
    imgs, programs = [], []
    for (h, w) in [(13, 9), (33, 47), (70, 130)]:
        for value in (0, 1, 127, 200, 255):
            for sigma in (0.13, 0.7, 1.5, 3.0):
                imgs.append(np.full((h, w, 3), value, dtype=np.uint8))
                programs.append([("GAUSS", sigma)])
    got, status, _ = run_raw(imgs, extra.pack_programs(programs))
    assert status == [0] * len(imgs)
    compare(got, imgs, programs)
    assert any((g != im).any() for g, im in zip(got, imgs))                        # the truncation case does occur (200 -> 198 at sigma 0.13)


def sampled():
    shapes = [SIZES[i % len(SIZES)] for i in range(16)]
    imgs = [image(h, w, 60 + i) for i, (h, w) in enumerate(shapes)]
    return imgs, extra.sample_extra(range(16), shapes)


def test_sixteen_sampled_programs_through_every_entrance():
    imgs, programs = sampled()
    ops = {s[0] for prog in programs for s in prog}
    assert ops == set(extra.OPS), ops                                              # seeds 0..15 draw every operation, all three blurs
    assert max(len(p) for p in programs) >= 5
    # the restatement alone: no NOISE byte of these programs lies within 1e-9 of an integer (observed: 0 of 60 417)
    assert sum(int(R.program_noise_mask(im, p).sum()) for im, p in zip(imgs, programs)) == 0
    got, status, _ = run_raw(imgs, extra.pack_programs(programs), calls=2)
    assert status == [0] * 16
    compare(got, imgs, programs)
    ref = R.extra_ref(imgs, programs)
    # the Python entrance: host arrays, separate GPU tensors, a mix, views into one allocation (the gather path)
    arena = torch.empty(sum(im.size + 256 for im in imgs), dtype=torch.uint8, device=DEV)
    views, pos = [], 0
    for im in imgs:
        v = arena[pos:pos + im.size].view(im.shape)
        v.copy_(torch.from_numpy(im))
        views.append(v)
        pos = (pos + im.size + 255) // 256 * 256
    on_gpu = [torch.from_numpy(im).to(DEV) for im in imgs]
    mixed = [g if i % 2 else im for i, (g, im) in enumerate(zip(on_gpu, imgs))]
    for what in (imgs, on_gpu, mixed, views):
        out = extra.extra_augment_batch(what, programs)
        assert all(o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() for o in out)
        assert len({o.untyped_storage().data_ptr() for o in out}) == 1             # what augment_batch's gather path asks for
        for o, r in zip(out, ref):
            assert np.array_equal(o.cpu().numpy(), r)
    assert all(np.array_equal(v.cpu().numpy(), im) for v, im in zip(views, imgs))


def test_a_malformed_program_is_reported_for_its_image_only():
    good = [("ADD", 3, 3, 3), ("MEDIAN", 3)]
    breakers = {
        "opcode": lambda r: r["steps"]["op"].__setitem__(0, 99),
        "median even": lambda r: r["steps"]["k"].__setitem__(1, 4),
        "median 13": lambda r: r["steps"]["k"].__setitem__(1, 13),
        "n_steps": lambda r: r.__setitem__("n_steps", 7),
        "add fraction": lambda r: r["steps"]["v"][0].__setitem__(0, 0.5),
    }
    gauss_breakers = {
        "sigma < 0": lambda r: r["steps"]["v"][0].__setitem__(0, -1.0),
        "sigma nan": lambda r: r["steps"]["v"][0].__setitem__(0, np.nan),
        "radius 13": lambda r: r["steps"]["v"][0].__setitem__(0, 3.2),
        "radius mismatch": lambda r: r.__setitem__("gauss_radius", 5),
        "weights": lambda r: r["gauss_w"].__setitem__(0, 0.5),
        "weights nan": lambda r: r["gauss_w"].__setitem__(1, np.nan),
    }
    other = {
        "average 8": ([("AVERAGE", 7)], lambda r: r["steps"]["k"].__setitem__(0, 8)),
        "average 1": ([("AVERAGE", 2)], lambda r: r["steps"]["k"].__setitem__(0, 1)),
        "scale < 0": ([("NOISE", 1.0, False, 1)], lambda r: r["steps"]["v"][0].__setitem__(0, -1.0)),
        "scale inf": ([("NOISE", 1.0, False, 1)], lambda r: r["steps"]["v"][0].__setitem__(0, np.inf)),
        "per_channel": ([("NOISE", 1.0, False, 1)], lambda r: r["steps"]["per_channel"].__setitem__(0, 2)),
        "mul nan": ([("MUL", 1.0, 1.0, 1.0)], lambda r: r["steps"]["v"][0].__setitem__(2, np.nan)),
        "alpha inf": ([("SHARPEN", 0.1, 1.0)], lambda r: r["steps"]["v"][0].__setitem__(0, np.inf)),
    }
    cases = [(good, None)]
    cases += [(good, f) for f in breakers.values()]
    cases += [([("GAUSS", 1.0)], None)]
    cases += [([("GAUSS", 1.0)], f) for f in gauss_breakers.values()]
    for prog, f in other.values():
        cases += [(prog, f), (prog, None)]
    imgs = [image(13, 9, 80 + i) if i % 2 else image(33, 47, 80 + i) for i in range(len(cases))]
    programs = [c[0] for c in cases]
    packed = extra.pack_programs(programs)
    for rec, (_, f) in zip(packed, cases):
        if f is not None:
            f(rec)
    got, status, _ = run_raw(imgs, packed)
    assert status == [0 if f is None else _ffi.EINVAL for _, f in cases]
    ref = R.extra_ref(imgs, programs)
    for g, r, im, (_, f) in zip(got, ref, imgs, cases):
        assert np.array_equal(g, im if f is not None else r)                       # passed through unchanged / untouched by its neighbour


def test_ranges_outside_their_buffers_and_host_arguments():
    lib = _ffi.lib()
    im = image(13, 9, 90)
    n = im.size
    src = torch.from_numpy(im.reshape(-1).copy()).to(DEV)
    packed = extra.pack_programs([[("ADD", 1, 1, 1)]] * 4)
    prog = torch.from_numpy(packed.view(np.uint8).reshape(-1).copy()).to(DEV)
    hw = torch.tensor([[13, 9]] * 3 + [[0, 9]], dtype=torch.int32, device=DEV)
    obuf, out = guarded(2 * n, 0x5A)
    wbuf, ws = guarded(2 * n, 0xA5)
    st = torch.full((4,), 12345, dtype=torch.int32, device=DEV)
    soff, ooff = dev_i64([0, 1, 0, 0]), dev_i64([0, n, n + 1, 0])                  # source 1 and output 2 end one byte too late
    args = [src.data_ptr(), n, soff.data_ptr(), hw.data_ptr(), prog.data_ptr(), 4, out.data_ptr(), 2 * n, ooff.data_ptr(),
            ws.data_ptr(), 2 * n, st.data_ptr(), _ffi.stream_ptr()]
    assert lib.yv3_extra_augment(*args) == 0
    torch.cuda.synchronize()
    assert st.tolist() == [0, _ffi.EINVAL, _ffi.EINVAL, _ffi.EINVAL]
    raw = out.cpu().numpy()
    assert np.array_equal(raw[:n], R.extra_ref([im], [[("ADD", 1, 1, 1)]])[0].reshape(-1)) and (raw[n:] == 0x5A).all()
    assert (obuf[:GUARD] == 0x5A).all().item() and (obuf[-GUARD:] == 0x5A).all().item() and (wbuf == 0xA5).all().item()

    # host arguments: refused before any launch (status and out keep their fill)
    out.fill_(0x5A)
    st.fill_(12345)
    for i in (0, 2, 3, 4, 6, 8, 9, 11):                                             # each pointer as NULL
        bad = list(args)
        bad[i] = None
        assert lib.yv3_extra_augment(*bad) == _ffi.EINVAL
    for i, v in ((1, 0), (1, -5), (5, 0), (5, -1), (5, 65536), (7, 0)):
        bad = list(args)
        bad[i] = v
        assert lib.yv3_extra_augment(*bad) == _ffi.EINVAL
    bad = list(args)
    bad[10] = 2 * n - 1
    assert lib.yv3_extra_augment(*bad) == _ffi.EWORKSPACE
    assert lib.yv3_extra_augment_workspace_bytes(0) == 0 and lib.yv3_extra_augment_workspace_bytes(-3) == 0
    torch.cuda.synchronize()
    assert st.tolist() == [12345] * 4 and (out == 0x5A).all().item()
    with pytest.raises(_ffi.Yv3Error) as e:                                        # the Python entrance checks on the host first
        extra.extra_augment_batch([im], [[("MEDIAN", 4)]])
    assert e.value.code == _ffi.EINVAL


def test_source_offsets_are_64_bit():
    far = 2 ** 31 + 12345
    arena = torch.empty(2 ** 31 + 2 ** 20, dtype=torch.uint8, device=DEV)          # allocated, not filled
    a, b = image(33, 47, 95), image(70, 130, 96)
    arena[far:far + a.size].copy_(torch.from_numpy(a.reshape(-1)))
    arena[0:b.size].copy_(torch.from_numpy(b.reshape(-1)))
    programs = [[("GAUSS", 1.5), ("ADD", 2, 2, 2)], [("MEDIAN", 5)]]
    views = [arena[far:far + a.size].view(a.shape), arena[0:b.size].view(b.shape)]
    out = extra.extra_augment_batch(views, programs)                               # two views into one allocation: gathered in place
    for o, r in zip(out, R.extra_ref([a, b], programs)):
        assert np.array_equal(o.cpu().numpy(), r)
    # a source that ends one byte past the allocation is refused, not read
    lib = _ffi.lib()
    prog = torch.from_numpy(extra.pack_programs(programs[:1]).view(np.uint8).reshape(-1).copy()).to(DEV)
    hw = torch.tensor([a.shape[:2]], dtype=torch.int32, device=DEV)
    res = torch.full((a.size,), 0x5A, dtype=torch.uint8, device=DEV)
    ws = torch.empty(a.size, dtype=torch.uint8, device=DEV)
    st = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
    zero = dev_i64([0])
    for off, code in ((arena.numel() - a.size + 1, _ffi.EINVAL), (far, 0)):
        soff = dev_i64([off])                                                      # (kept alive across the call)
        _ffi.check(lib.yv3_extra_augment(arena.data_ptr(), arena.numel(), soff.data_ptr(), hw.data_ptr(), prog.data_ptr(), 1,
                                         res.data_ptr(), a.size, zero.data_ptr(), ws.data_ptr(), a.size, st.data_ptr(),
                                         _ffi.stream_ptr()))
        torch.cuda.synchronize()
        assert st.tolist() == [code]
        assert (res == 0x5A).all().item() if code else np.array_equal(res.cpu().numpy().reshape(a.shape), R.extra_ref([a], programs[:1])[0])


# ---- the loader ---------------------------------------------------------------------------------------------------------------------
LOADER_SHAPES = [(60, 80), (45, 35), (33, 47), (8, 8), (45, 35), (70, 130), (60, 80)]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("extra_loader")
    (root / "images").mkdir()
    (root / "labels").mkdir()
    rng = np.random.RandomState(31)
    paths = []
    for i, (h, w) in enumerate(LOADER_SHAPES):
        p = str(root / "images" / ("img%d.jpg" % i))
        Image.fromarray(image(h, w, 100 + i)).save(p, format="JPEG", quality=90)
        paths.append(p)
        rows = np.column_stack([rng.randint(0, 3, 3), rng.uniform(0.3, 0.7, (3, 2)), rng.uniform(0.2, 0.5, (3, 2))])
        np.savetxt(str(root / "labels" / ("img%d.txt" % i)), rows)
    lst = root / "train.txt"
    lst.write_text("\n".join(paths) + "\n")
    return str(lst), paths


def epochs(loader, n):
    return [[(x.cpu().numpy(), t.cpu().numpy()) for x, t in loader] for _ in range(n)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.int32), x0.view(np.int32)) and np.array_equal(t.view(np.int32), t0.view(np.int32))
                                    for (x, t), (x0, t0) in zip(a, b))


def test_train_batches_with_extra(listing):
    lst, paths = listing
    kw = dict(seed=4, jitter=0.2)
    base = epochs(aug.TrainBatches(lst, 3, (128, 96), extra=True, **kw), 2)
    assert [len(e) for e in base] == [3, 3]
    # every batch of the first epoch is augment_batch(extra_ref(...)) of the same draws
    order, seeds, _ = aug.epoch_schedule(4, 0, len(paths), 3)
    for k in range(3):
        idx = [int(j) for j in order[3 * k:3 * k + 3]]
        srcs = [evaluate.read_image_rgb(paths[j]) for j in idx]
        shapes = [s.shape[:2] for s in srcs]
        programs = extra.sample_extra(seeds[3 * k:3 * k + 3], shapes)
        params = aug.sample_params(seeds[3 * k:3 * k + 3], shapes=shapes, jitter=0.2)
        for im, p in zip(srcs, programs):
            assert not R.program_noise_mask(im, p).any()
        x, t = aug.augment_batch(R.extra_ref(srcs, programs), [aug.read_labels(aug.label_path(paths[j])) for j in idx], (128, 96), params)
        assert same([base[0][k]], [(x.cpu().numpy(), t.cpu().numpy())])
    # the same bits with decode threads, with the arena (second epoch: every source resident, gathered in place), with GPU decode
    full = aug.TrainBatches(lst, 3, (128, 96), **kw).decoded_bytes()
    for conf in (dict(workers=3, prefetch=2), dict(cache_bytes=full), dict(cache_bytes=full // 2, workers=2), dict(decode="gpu"),
                 dict(decode="gpu", cache_bytes=full)):
        loader = aug.TrainBatches(lst, 3, (128, 96), extra=True, **kw, **conf)
        got = epochs(loader, 2)
        assert same(got[0], base[0]) and same(got[1], base[1]), conf
        if conf.get("cache_bytes") == full:
            assert loader.resident_images() == len(paths)
    # across a resume
    loader = aug.TrainBatches(lst, 3, (128, 96), extra=True, **kw)
    it = iter(loader)
    next(it)
    state = loader.state_dict()
    assert state["config"]["extra"] is True
    it.close()
    fresh = aug.TrainBatches(lst, 3, (128, 96), extra=True, **kw)
    fresh.load_state_dict(state)
    assert same(epochs(fresh, 1)[0], base[0][1:])
    with pytest.raises(ValueError):
        aug.TrainBatches(lst, 3, (128, 96), **kw).load_state_dict(state)
    # off: the loader is what it was, and its state dict carries no new key
    plain, off = aug.TrainBatches(lst, 3, (128, 96), **kw), aug.TrainBatches(lst, 3, (128, 96), extra=False, **kw)
    assert "extra" not in off.state_dict()["config"] and off.state_dict() == plain.state_dict()
    a, b = epochs(plain, 1)[0], epochs(off, 1)[0]
    assert same(a, b) and not same(a, base[0])
    off.load_state_dict(plain.state_dict())
