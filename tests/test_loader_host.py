"""The host half of the training loader (yolo_v3_amd/augment.py): the epoch schedule and its multi-scale dims, decoding ahead on
worker threads, the arena's admission rule and the resume state.  Nothing here touches a GPU."""

import threading
import time

import numpy as np
import pytest

from yolo_v3_amd import augment as aug
from yolo_v3_amd import evaluate


# ---- schedule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffle", [True, False])
def test_schedule_equals_the_restated_streams(shuffle):
    for seed, epoch, n, bs in [(4, 0, 5, 2), (7, 3, 64, 16), (0, 1, 1, 3)]:
        order, seeds, dims = aug.epoch_schedule(seed, epoch, n, bs, shuffle=shuffle)
        rng = np.random.RandomState([seed, epoch])
        ref_order = rng.permutation(n) if shuffle else np.arange(n)
        ref_seeds = rng.randint(0, 2 ** 31 - 1, size=n)
        assert np.array_equal(order, ref_order) and np.array_equal(seeds, ref_seeds)
        assert dims is None


def test_schedule_multiscale():
    n, bs, interval = 103, 4, 3
    n_batches = 26
    base = aug.epoch_schedule(9, 2, n, bs)
    order, seeds, dims = aug.epoch_schedule(9, 2, n, bs, multiscale=(64, 128), dim_interval=interval)
    assert np.array_equal(order, base[0]) and np.array_equal(seeds, base[1])      # switching dims on moves no other draw
    assert len(dims) == n_batches
    for k, (w, h) in enumerate(dims):
        assert w == h and w % 32 == 0 and 64 <= w <= 128
        assert (w, h) == dims[k // interval * interval]                            # constant over each run of `interval` batches
    # the documented draw, after the seeds
    rng = np.random.RandomState([9, 2])
    rng.permutation(n)
    rng.randint(0, 2 ** 31 - 1, size=n)
    steps = rng.randint(64 // 32, 128 // 32 + 1, size=9) * 32
    assert [d[0] for d in dims] == [int(steps[k // interval]) for k in range(n_batches)]
    again = aug.epoch_schedule(9, 2, n, bs, multiscale=(64, 128), dim_interval=interval)[2]
    other = aug.epoch_schedule(9, 3, n, bs, multiscale=(64, 128), dim_interval=interval)[2]
    assert again == dims and other != dims
    # 320..608 in steps of 32: all ten values occur
    wide = aug.epoch_schedule(1, 0, 2000, 1, multiscale=(320, 608), dim_interval=1)[2]
    assert len(wide) == 2000 and sorted(set(w for w, _ in wide)) == list(range(320, 609, 32))
    # a single value is allowed
    assert set(aug.epoch_schedule(1, 0, 10, 2, multiscale=(96, 96))[2]) == {(96, 96)}
    for bad in [(100, 128), (64, 100), (128, 64), (0, 64), (-32, 64)]:
        with pytest.raises(ValueError):
            aug.epoch_schedule(1, 0, 10, 2, multiscale=bad)
    with pytest.raises(ValueError):
        aug.epoch_schedule(1, 0, 10, 2, multiscale=(64, 128), dim_interval=0)


# ---- admission ----------------------------------------------------------------------------------------------------------------
def test_arena_admission_rule():
    offsets, end = aug.arena_admit([300, 256, 1000, 10], 1024)
    assert offsets == [0, 512, None, 768] and end == 778
    assert aug.arena_admit([300, 256, 1000, 10], 1024) == (offsets, end)           # deterministic
    assert aug.arena_admit([10], 1024, start=end) == ([None], end)                 # 1024 + 10 > 1024
    assert aug.arena_admit([256], 1024, start=300) == ([512], 768)                 # continues at the next aligned offset
    assert aug.arena_admit([1024, 1], 1024) == ([0, None], 1024)                   # an exact fit
    assert aug.arena_admit([], 0) == ([], 0)


# ---- a list file on disk --------------------------------------------------------------------------------------------------------
SHAPES = [(12, 16), (9, 7), (1, 1), (33, 47), (8, 8), (20, 10), (5, 31)]


@pytest.fixture
def listing(tmp_path):
    from PIL import Image
    (tmp_path / "images").mkdir()
    (tmp_path / "labels").mkdir()
    rng = np.random.RandomState(3)
    paths = []
    for i, (h, w) in enumerate(SHAPES):
        p = str(tmp_path / "images" / ("img%d.jpg" % i))                           # PNG bytes under the reference's .jpg naming
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(p, format="PNG")
        paths.append(p)
        if i != 2:                                                                 # image 2 has no label file
            np.savetxt(str(tmp_path / "labels" / ("img%d.txt" % i)), rng.uniform(0.2, 0.6, (1 + i % 3, 5)))
    lst = tmp_path / "train.txt"
    lst.write_text("\n".join(paths) + "\n")
    return str(lst), paths


def collect(gen):
    return [([im.copy() for im in images], [l.copy() for l in labels], params.copy(), dim) for images, labels, params, dim in gen]


def same_batches(a, b):
    assert len(a) == len(b)
    for (ia, la, pa, da), (ib, lb, pb, db) in zip(a, b):
        assert len(ia) == len(ib) and all(np.array_equal(x, y) for x, y in zip(ia, ib))
        assert all(np.array_equal(x, y) for x, y in zip(la, lb))
        assert np.array_equal(pa, pb) and da == db


def pool_threads():
    return [t for t in threading.enumerate() if t.name.startswith("yv3-decode")]


def test_decode_ahead_gives_the_same_batches_in_order(listing, monkeypatch):
    lst, _ = listing
    real = evaluate.read_image_rgb
    delay = np.random.RandomState(5)
    lock = threading.Lock()

    def slow(path):
        with lock:
            d = delay.uniform(0.0, 0.02)
        time.sleep(d)                                                              # decodes finish out of order
        return real(path)

    plain = collect(aug.TrainBatches(lst, 3, (64, 64), seed=2, jitter=0.2).host_batches())
    assert [len(b[0]) for b in plain] == [3, 3, 1]
    monkeypatch.setattr(evaluate, "read_image_rgb", slow)
    ahead = collect(aug.TrainBatches(lst, 3, (64, 64), seed=2, jitter=0.2, workers=4, prefetch=3).host_batches())
    same_batches(plain, ahead)
    assert not pool_threads()
    # the host half is the documented streams
    order, seeds, _ = aug.epoch_schedule(2, 0, 7, 3)
    for k, (images, labels, params, dim) in enumerate(plain):
        idx = order[3 * k:3 * k + 3]
        assert [im.shape[:2] for im in images] == [SHAPES[j] for j in idx] and dim == (64, 64)
        assert np.array_equal(params, aug.sample_params(seeds[3 * k:3 * k + 3], shapes=[SHAPES[j] for j in idx], jitter=0.2))
        assert [len(l) for l in labels] == [0 if j == 2 else 1 + j % 3 for j in idx]


@pytest.mark.parametrize("workers", [0, 4])
def test_a_missing_image_raises_at_its_own_batch(listing, workers):
    import os
    lst, paths = listing
    os.remove(paths[4])
    loader = aug.TrainBatches(lst, 3, (64, 64), seed=2, shuffle=False, workers=workers, prefetch=3)
    gen = loader.host_batches()
    first = next(gen)                                                              # images 0..2: delivered
    assert [im.shape[:2] for im in first[0]] == SHAPES[:3]
    with pytest.raises(FileNotFoundError):
        next(gen)                                                                  # images 3..5
    assert not pool_threads()                                                      # the failed generator has joined its pool


def test_close_joins_the_pool(listing):
    lst, _ = listing
    gen = aug.TrainBatches(lst, 1, (64, 64), seed=2, workers=4, prefetch=3).host_batches()
    next(gen)
    assert pool_threads()
    gen.close()
    assert not pool_threads()
    # dropping the iterator does the same
    gen = aug.TrainBatches(lst, 1, (64, 64), seed=2, workers=4, prefetch=3).host_batches()
    next(gen)
    del gen
    assert not pool_threads()


def test_workers_are_capped(listing):
    lst, _ = listing
    assert aug.TrainBatches(lst, 1, (64, 64), seed=2, workers=1000).workers == 16
    assert aug.TrainBatches(lst, 1, (64, 64), seed=2).workers == 0


def test_new_keywords_do_not_reach_sample_params(listing):
    lst, _ = listing
    loader = aug.TrainBatches(lst, 2, (64, 64), seed=1, multiscale=(64, 128), dim_interval=2, workers=2, prefetch=1, cache_bytes=0,
                              jitter=0.1, hue=0.05)
    assert loader.aug == {"jitter": 0.1, "hue": 0.05}
    dims = [b[3] for b in loader.host_batches()]
    assert dims == aug.epoch_schedule(1, 0, 7, 2, multiscale=(64, 128), dim_interval=2)[2]
    with pytest.raises(ValueError):
        aug.TrainBatches(lst, 2, (64, 64), seed=1, multiscale=(64, 100))


def test_decoded_bytes(listing):
    lst, _ = listing
    assert aug.TrainBatches(lst, 2, (64, 64), seed=1).decoded_bytes() == sum((h * w * 3 + 255) // 256 * 256 for h, w in SHAPES)


# ---- resume -------------------------------------------------------------------------------------------------------------------
def test_state_round_trip(listing):
    lst, _ = listing
    kw = dict(multiscale=(64, 128), dim_interval=2, jitter=0.2)
    loader = aug.TrainBatches(lst, 2, (64, 64), seed=6, **kw)
    s0 = loader.state_dict()
    assert (s0["seed"], s0["epoch"], s0["batch"]) == (6, 0, 0)
    assert s0["config"] == {"n": 7, "batch_size": 2, "shuffle": True, "multiscale": [64, 128], "dim_interval": 2, "aug": {"jitter": 0.2}}
    first = collect(loader.host_batches())
    assert loader.state_dict()["epoch"] == 0 and loader.state_dict()["batch"] == 4     # complete
    gen = loader.host_batches()
    head = collect(next(gen) for _ in range(2))
    state = loader.state_dict()
    assert (state["epoch"], state["batch"]) == (1, 2)
    tail = collect(gen)

    fresh = aug.TrainBatches(lst, 2, (64, 64), seed=0, **kw)                        # the seed comes from the state
    fresh.load_state_dict(state)
    assert fresh.state_dict() == state
    same_batches(collect(fresh.host_batches()), tail)
    assert fresh.state_dict()["epoch"] == 1 and fresh.state_dict()["batch"] == 4
    third = collect(fresh.host_batches())                                           # then the next epoch, as the original does
    same_batches(third, collect(loader.host_batches()))

    # a complete epoch resumes at the next one; batch 0 repeats the epoch
    done = aug.TrainBatches(lst, 2, (64, 64), seed=6, **kw)
    done.load_state_dict(dict(state, epoch=0, batch=4))
    same_batches(collect(done.host_batches()), head + tail)
    again = aug.TrainBatches(lst, 2, (64, 64), seed=6, **kw)
    again.load_state_dict(s0)
    same_batches(collect(again.host_batches()), first)


def test_state_of_another_config_raises(listing):
    lst, _ = listing
    state = aug.TrainBatches(lst, 2, (64, 64), seed=6, jitter=0.2).state_dict()
    for other in (dict(batch_size=3, jitter=0.2), dict(batch_size=2, jitter=0.3), dict(batch_size=2, jitter=0.2, shuffle=False),
                  dict(batch_size=2, jitter=0.2, multiscale=(64, 128)), dict(batch_size=2)):
        bs = other.pop("batch_size")
        with pytest.raises(ValueError):
            aug.TrainBatches(lst, bs, (64, 64), seed=6, **other).load_state_dict(state)
    with pytest.raises(ValueError):
        aug.TrainBatches(lst, 2, (64, 64), seed=6, jitter=0.2).load_state_dict(dict(state, batch=5))
