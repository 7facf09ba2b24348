"""The training loader on the GPU: yv3_augment_images_from (sources gathered from a resident arena, csrc/augment.hip) against the packed
entry point and the numpy restatement tests/augment_ref.py, bit for bit, with guard bytes, offsets beyond 2^31 and the error codes;
then TrainBatches with decode-ahead, the arena, resume and multi-scale dims: every configuration yields the same bits."""

import collections

import numpy as np
import pytest
import torch

from tests import augment_ref as A
from tests.helpers import trained_like_stream
from yolo_v3_amd import YoloNet, WeightManager, _ffi, evaluate
from yolo_v3_amd import augment as aug

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096


def images(shapes, seed):
    rng = np.random.RandomState(seed)
    out = []
    for (h, w) in shapes:
        yy, xx = np.mgrid[0:h, 0:w]                                                # colour ramps plus noise: every hue sector occurs
        base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 97) % 256], -1)
        out.append(np.clip(base + rng.randint(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


def extreme_params(shapes, k):
    """Rows at the ends of darknet's ranges: every side -0.3 or +0.3, dsat / dexp at 1/1.5 and 1.5, |dhue| = 17.9, flips."""
    rows = []
    for i, (h, w) in enumerate(shapes):
        j = i + k
        sgn = [1 if (j >> b) & 1 else -1 for b in range(4)]
        sides = [np.rint(0.3 * n) * s for n, s in zip((h, w, h, w), sgn)]
        sides[0], sides[2] = aug.keep_one_pixel(sides[0], sides[2], h)
        sides[3], sides[1] = aug.keep_one_pixel(sides[3], sides[1], w)
        rows.append([17.9 if j % 2 else -17.9, 1.5 if j % 3 else 1 / 1.5, 1 / 1.5 if j % 4 < 2 else 1.5] + sides + [float(j % 2)])
    return np.array(rows, dtype=np.float64)


def guarded(n, dtype, fill):
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def dev_i64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def call_from(lib, src, src_bytes, src_off, ws_off, ws_span, hw, params, B, out, oh, ow, ws, ws_bytes, st):
    ptr = lambda t: None if t is None else t.data_ptr()
    return lib.yv3_augment_images_from(ptr(src), src_bytes, ptr(src_off), ptr(ws_off), ws_span, ptr(hw), ptr(params), B, ptr(out), oh, ow,
                                       ptr(ws), ws_bytes, ptr(st), _ffi.stream_ptr())


# ---- 1. the entry point ---------------------------------------------------------------------------------------------------------
def test_gathering_entry_point_equals_the_packed_one():
    shapes = [(1, 1), (5, 7), (33, 47), (64, 64)]
    srcs = images(shapes, 21)
    batch = [2, 0, 3, 2, 1]                                                        # the (33, 47) source occurs twice
    B, OH, OW = len(batch), 64, 96
    bshapes = [shapes[j] for j in batch]
    params = extreme_params(bshapes, 5)
    # the arena: sources in scrambled order at odd offsets, noise in between
    place, pos = {}, 7
    for j in (3, 1, 0, 2):
        place[j] = pos
        pos = (pos + srcs[j].size + 1000) | 1
    arena_np = np.random.RandomState(22).randint(0, 256, pos + 333).astype(np.uint8)
    for j, off in place.items():
        assert off % 2 == 1
        arena_np[off:off + srcs[j].size] = srcs[j].reshape(-1)
    arena = torch.from_numpy(arena_np).to(DEV)
    src_off = [place[j] for j in batch]
    ws_off, ws_span = [], 0
    for j in batch:                                                                # compact, unaligned
        ws_off.append(ws_span)
        ws_span += srcs[j].size
    assert any(o % 256 for o in ws_off[1:])
    hw = torch.tensor(bshapes, dtype=torch.int32, device=DEV)
    par = torch.from_numpy(params).to(DEV)
    lib = _ffi.lib()
    xbuf, x = guarded(B * 3 * OH * OW, torch.float32, -7.0)
    wbuf, ws = guarded(ws_span, torch.uint8, 0xA5)
    sbuf, st = guarded(B, torch.int32, 12345)
    _ffi.check(call_from(lib, arena, arena.numel(), dev_i64(src_off), dev_i64(ws_off), ws_span, hw, par, B, x, OH, OW, ws, ws_span, st))
    torch.cuda.synchronize()
    for buf, fill in ((xbuf, -7.0), (wbuf, 0xA5), (sbuf, 12345)):
        assert (buf[:GUARD] == fill).all().item() and (buf[-GUARD:] == fill).all().item()
    assert st.tolist() == [0] * B
    assert not (x == -7.0).any().item()                                            # every output element written
    assert np.array_equal(arena.cpu().numpy(), arena_np)                           # the sources are only read
    got = x.view(B, 3, OH, OW).cpu().numpy()

    # the packed entry point on a packed copy
    offs, pos = [], 0
    for j in batch:
        offs.append(pos)
        pos += (srcs[j].size + 255) // 256 * 256
    flat = np.zeros(pos, dtype=np.uint8)
    for o, j in zip(offs, batch):
        flat[o:o + srcs[j].size] = srcs[j].reshape(-1)
    packed = torch.from_numpy(flat).to(DEV)
    x2 = torch.empty((B, 3, OH, OW), device=DEV)
    ws2 = torch.empty(pos, dtype=torch.uint8, device=DEV)
    st2 = torch.empty(B, dtype=torch.int32, device=DEV)
    _ffi.check(lib.yv3_augment_images(packed.data_ptr(), pos, dev_i64(offs).data_ptr(), hw.data_ptr(), par.data_ptr(), B, x2.data_ptr(),
                                      OH, OW, ws2.data_ptr(), pos, st2.data_ptr(), _ffi.stream_ptr()))
    torch.cuda.synchronize()
    assert st2.tolist() == [0] * B
    assert np.array_equal(got.view(np.int32), x2.cpu().numpy().view(np.int32))
    for b, j in enumerate(batch):
        assert np.array_equal(got[b], A.augment_image(srcs[j], params[b], (OW, OH))), "image %d" % b
    assert not np.array_equal(got[0], got[3])                                       # the two (33, 47) rows have their own parameters


# ---- 2. offsets beyond 2^31 -------------------------------------------------------------------------------------------------------
def test_offsets_are_64_bit():
    far = 2 ** 31 + 12345
    arena = torch.empty(2 ** 31 + 2 ** 20, dtype=torch.uint8, device=DEV)           # allocated, not filled
    a, b = images([(33, 47), (33, 47)], 23)
    arena[far:far + a.size].copy_(torch.from_numpy(a.reshape(-1)))
    arena[0:b.size].copy_(torch.from_numpy(b.reshape(-1)))
    params = extreme_params([(33, 47)] * 2, 2)
    hw = torch.tensor([(33, 47)] * 2, dtype=torch.int32, device=DEV)
    par = torch.from_numpy(params).to(DEV)
    x = torch.full((2, 3, 64, 96), -7.0, device=DEV)
    ws_span = 2 * a.size
    ws = torch.empty(ws_span, dtype=torch.uint8, device=DEV)
    st = torch.full((2,), 12345, dtype=torch.int32, device=DEV)
    _ffi.check(call_from(_ffi.lib(), arena, arena.numel(), dev_i64([far, 0]), dev_i64([0, a.size]), ws_span, hw, par, 2, x, 64, 96, ws,
                         ws_span, st))
    torch.cuda.synchronize()
    assert st.tolist() == [0, 0]
    got = x.cpu().numpy()
    assert np.array_equal(got[0], A.augment_image(a, params[0], (96, 64)))
    assert np.array_equal(got[1], A.augment_image(b, params[1], (96, 64)))
    # the same through augment_batch: two views into the big allocation take the gather path
    views = [arena[far:far + a.size].view(33, 47, 3), arena[0:b.size].view(33, 47, 3)]
    xb, _ = aug.augment_batch(views, None, (96, 64), params)
    assert np.array_equal(xb.cpu().numpy(), got)
    # a source that ends one byte past the allocation is refused, not read
    _ffi.check(call_from(_ffi.lib(), arena, arena.numel(), dev_i64([arena.numel() - a.size + 1, 0]), dev_i64([0, a.size]), ws_span, hw, par,
                         2, x, 64, 96, ws, ws_span, st))
    torch.cuda.synchronize()
    assert st.tolist() == [_ffi.EINVAL, 0] and not x[0].any().item()


# ---- 3. error codes -------------------------------------------------------------------------------------------------------------
def test_error_codes():
    imgs = images([(20, 30), (40, 10)], 24)
    sizes = [im.size for im in imgs]
    good = np.array([[0, 1, 1, 0, 0, 0, 0, 0]] * 2, dtype=np.float64)
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(DEV)
    src_bytes = ws_span = sum(sizes)
    offs = dev_i64([0, sizes[0]])
    hw = torch.tensor([im.shape[:2] for im in imgs], dtype=torch.int32, device=DEV)
    par = torch.from_numpy(good).to(DEV)
    x = torch.empty((2, 3, 64, 64), device=DEV)
    ws = torch.empty(ws_span, dtype=torch.uint8, device=DEV)
    st = torch.empty(2, dtype=torch.int32, device=DEV)
    lib = _ffi.lib()

    def call(**kw):
        a = dict(src=src, src_bytes=src_bytes, src_off=offs, ws_off=offs, ws_span=ws_span, hw=hw, params=par, B=2, out=x, oh=64, ow=64,
                 ws=ws, wsb=ws_span, st=st)
        a.update(kw)
        return call_from(lib, a["src"], a["src_bytes"], a["src_off"], a["ws_off"], a["ws_span"], a["hw"], a["params"], a["B"], a["out"],
                         a["oh"], a["ow"], a["ws"], a["wsb"], a["st"])

    assert call() == 0
    torch.cuda.synchronize()
    assert st.tolist() == [0, 0]
    ref = [A.augment_image(im, p, (64, 64)) for im, p in zip(imgs, good)]
    assert np.array_equal(x[0].cpu().numpy(), ref[0]) and np.array_equal(x[1].cpu().numpy(), ref[1])
    for kw in (dict(src=None), dict(src_off=None), dict(ws_off=None), dict(hw=None), dict(params=None), dict(out=None), dict(ws=None),
               dict(st=None), dict(B=0), dict(B=-1), dict(oh=0), dict(ow=-5), dict(src_bytes=0), dict(src_bytes=-1), dict(ws_span=0),
               dict(ws_span=-4)):
        assert call(**kw) == _ffi.EINVAL, kw
    assert call(wsb=ws_span - 1) == _ffi.EWORKSPACE
    # a range past its bound: found on the device, that image's outputs are zeros and the other image is right
    for kw in (dict(src_off=dev_i64([0, src_bytes - sizes[1] + 1])), dict(src_off=dev_i64([0, -1])),
               dict(ws_off=dev_i64([0, ws_span - sizes[1] + 1])), dict(ws_off=dev_i64([0, -1])),
               dict(ws_off=dev_i64([0, 2 ** 62]))):
        x.fill_(-1.0)
        st.fill_(777)
        assert call(**kw) == 0
        torch.cuda.synchronize()
        assert st.tolist() == [0, _ffi.EINVAL]
        assert not x[1].any().item() and np.array_equal(x[0].cpu().numpy(), ref[0])


# ---- 4-6. the loader ------------------------------------------------------------------------------------------------------------
LOADER_SHAPES = [(120, 160), (90, 70), (1, 1), (33, 47), (90, 70), (33, 47), (120, 160)]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("loader")
    (root / "images").mkdir()
    (root / "labels").mkdir()
    rng = np.random.RandomState(31)
    paths = []
    for i, im in enumerate(images(LOADER_SHAPES, 30)):
        p = str(root / "images" / ("img%d.jpg" % i))                               # PNG bytes under the reference's .jpg naming: lossless
        Image.fromarray(im).save(p, format="PNG")
        paths.append(p)
        if i != 2:                                                                 # image 2 has no label file
            rows = np.column_stack([rng.randint(0, 3, 4), rng.uniform(0.3, 0.7, (4, 2)), rng.uniform(0.2, 0.5, (4, 2))])
            np.savetxt(str(root / "labels" / ("img%d.txt" % i)), rows)
    lst = root / "train.txt"
    lst.write_text("\n".join(paths) + "\n")
    return str(lst)


class CountingLib:
    """libyv3 with the calls of the two pixel entry points counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("yv3_augment_images", "yv3_augment_images_from"):
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def run_epochs(lst, n_epochs, **kw):
    loader = aug.TrainBatches(lst, 3, (128, 96), seed=4, jitter=0.2, **kw)
    out = []
    for _ in range(n_epochs):
        out.append([(x.cpu().numpy(), t.cpu().numpy()) for x, t in loader])
    return loader, out


def test_one_loader_every_path(listing, monkeypatch):
    lib = CountingLib(_ffi.lib())
    monkeypatch.setattr(_ffi, "lib", lambda: lib)
    reads = []                                                                     # (list.append is atomic: workers call this too)
    real = evaluate.read_image_rgb

    def counting_read(path):
        reads.append(path)
        return real(path)
    monkeypatch.setattr(evaluate, "read_image_rgb", counting_read)

    _, base = run_epochs(listing, 2)
    assert [len(e) for e in base] == [3, 3] and [b[0].shape for b in base[0]] == [(3, 3, 96, 128), (3, 3, 96, 128), (1, 3, 96, 128)]
    assert lib.calls == {"yv3_augment_images": 6} and len(reads) == 14
    assert any(b[1].any() for b in base[0])                                         # label rows arrive
    full = aug.TrainBatches(listing, 3, (128, 96), seed=4).decoded_bytes()
    assert full == sum((h * w * 3 + 255) // 256 * 256 for h, w in LOADER_SHAPES)
    partial = 3 * 19200                                                            # one (120, 160) source, or three (90, 70)
    configs = [dict(workers=3, prefetch=2), dict(cache_bytes=full), dict(cache_bytes=partial), dict(cache_bytes=full, workers=3, prefetch=2)]
    for kw in configs:
        lib.calls.clear()
        reads.clear()
        loader = aug.TrainBatches(listing, 3, (128, 96), seed=4, jitter=0.2, **kw)
        got = []
        for epoch in range(2):
            got.append([(x.cpu().numpy(), t.cpu().numpy()) for x, t in loader])
            if epoch == 0:
                first_reads, first_calls = len(reads), dict(lib.calls)
        for e in range(2):
            assert len(got[e]) == 3
            for (x, t), (x0, t0) in zip(got[e], base[e]):
                assert np.array_equal(x.view(np.int32), x0.view(np.int32)) and np.array_equal(t.view(np.int32), t0.view(np.int32)), kw
        assert first_reads == 7
        second_calls = {k: v - first_calls.get(k, 0) for k, v in lib.calls.items()}
        if kw.get("cache_bytes") == full:
            assert len(reads) == 7                                                  # nothing is read or decoded in the second epoch
            assert loader.resident_images() == 7
            assert second_calls.get("yv3_augment_images_from") == 3 and not second_calls.get("yv3_augment_images")
        elif kw.get("cache_bytes"):
            assert 0 < loader.resident_images() < 7 and len(reads) == 14 - loader.resident_images()
        else:
            assert len(reads) == 14 and not lib.calls.get("yv3_augment_images_from")
    # the restatement, once: the first batch of the first epoch
    order, seeds, _ = aug.epoch_schedule(4, 0, 7, 3)
    srcs = images(LOADER_SHAPES, 30)
    params = aug.sample_params(seeds[:3], shapes=[LOADER_SHAPES[j] for j in order[:3]], jitter=0.2)
    for i, j in enumerate(order[:3]):
        assert np.array_equal(base[0][0][0][i], A.augment_image(srcs[j], params[i], (128, 96)))


def test_resume_continues_the_epoch(listing):
    kw = dict(multiscale=(64, 128), dim_interval=2, jitter=0.2, cache_bytes=1 << 20)
    loader = aug.TrainBatches(listing, 2, (128, 96), seed=8, **kw)
    for _ in loader:
        pass
    it = iter(loader)
    next(it), next(it)
    state = loader.state_dict()
    assert (state["epoch"], state["batch"]) == (1, 2)
    rest = [(x.cpu().numpy(), t.cpu().numpy()) for x, t in it]
    assert len(rest) == 2
    fresh = aug.TrainBatches(listing, 2, (128, 96), seed=8, multiscale=(64, 128), dim_interval=2, jitter=0.2)
    fresh.load_state_dict(state)
    again = [(x.cpu().numpy(), t.cpu().numpy()) for x, t in fresh]
    dims = aug.epoch_schedule(8, 1, 7, 2, multiscale=(64, 128), dim_interval=2)[2]
    assert len(again) == 2
    for k, ((x, t), (x0, t0)) in enumerate(zip(again, rest)):
        assert x.shape[2:] == (dims[2 + k][1], dims[2 + k][0]) and x.shape == x0.shape
        assert np.array_equal(x.view(np.int32), x0.view(np.int32)) and np.array_equal(t.view(np.int32), t0.view(np.int32))


def test_multiscale_batches_into_a_training_step(listing):
    C = 3
    seed = next(s for s in range(100) if len(set(aug.epoch_schedule(s, 0, 7, 2, multiscale=(64, 128), dim_interval=1)[2][:3])) >= 2)
    dims = aug.epoch_schedule(seed, 0, 7, 2, multiscale=(64, 128), dim_interval=1)[2]
    net = YoloNet((96, 96), numClass=C)
    WeightManager(net).load_stream(trained_like_stream(C))
    net = net.to(DEV).train()
    net.backprop = True
    loader = aug.TrainBatches(listing, 2, (96, 96), seed=seed, multiscale=(64, 128), dim_interval=1, jitter=0.2)
    seen = set()
    for k, (x, target) in zip(range(3), loader):
        assert tuple(x.shape) == (2, 3, dims[k][1], dims[k][0])
        seen.add(tuple(x.shape[2:]))
        net.zero_grad()
        loss = net(x, target)
        loss.backward()
        assert torch.isfinite(loss).item()
        for name, p in net.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and torch.isfinite(p.grad).all().item(), (name, dims[k])
    assert len(seen) >= 2
