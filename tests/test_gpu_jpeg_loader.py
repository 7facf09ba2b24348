"""``decode="gpu"`` in the training loader and the results writer: eight small JPEGs, and every configuration of `TrainBatches`
(defaults, workers, a full and a partial arena, resume) and `generate_results_file` gives the bits ``decode="pil"`` gives."""
import numpy as np
import pytest

from tests.helpers import load_sw1_net
from tests.test_jpeg_host import picture
from yolo_v3_amd import evaluate, jpeg, synth
from yolo_v3_amd import augment as aug

pytestmark = pytest.mark.gpu

# (w, h), save options: every sampling, a grey file, restart markers, and one progressive file that takes the PIL path
FILES = [((120, 90), dict(subsampling=2)), ((70, 90), dict(subsampling=1, restart_marker_blocks=3)), ((64, 64), dict(subsampling=0)),
         ((33, 47), dict(subsampling=2, optimize=True)), ((160, 120), dict(subsampling=2, restart_marker_rows=1)), ((57, 31), dict()),
         ((96, 80), dict(progressive=True)), ((81, 99), dict(subsampling=1))]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    root = tmp_path_factory.mktemp("jpeg_loader")
    (root / "images").mkdir()
    (root / "labels").mkdir()
    rng = np.random.RandomState(41)
    paths = []
    for i, ((w, h), kw) in enumerate(FILES):
        p = str(root / "images" / ("img%d.jpg" % i))
        picture(w, h, "L" if i == 5 else "RGB", "gradient" if i % 2 else "noise", seed=50 + i).save(p, "JPEG", quality=85, **kw)
        paths.append(p)
        if i != 2:                                                                 # image 2 has no label file
            rows = np.column_stack([rng.randint(0, 3, 4), rng.uniform(0.3, 0.7, (4, 2)), rng.uniform(0.2, 0.5, (4, 2))])
            np.savetxt(str(root / "labels" / ("img%d.txt" % i)), rows)
    lst = root / "train.txt"
    lst.write_text("\n".join(paths) + "\n")
    return str(lst)


def epochs(lst, n, **kw):
    loader = aug.TrainBatches(lst, 3, (128, 96), seed=4, jitter=0.2, **kw)
    return loader, [[(x.cpu().numpy(), t.cpu().numpy()) for x, t in loader] for _ in range(n)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.int32), x0.view(np.int32)) and np.array_equal(t.view(np.int32), t0.view(np.int32))
                                    for (x, t), (x0, t0) in zip(a, b))


def test_train_batches_yield_the_same_bits(listing, monkeypatch):
    _, base = epochs(listing, 2)                                                   # decode="pil", the default
    assert [len(e) for e in base] == [3, 3] and any(b[1].any() for b in base[0])
    reads = []
    real = evaluate.read_image_rgb

    def counting_read(path):
        reads.append(path)
        return real(path)
    monkeypatch.setattr(evaluate, "read_image_rgb", counting_read)
    full = aug.TrainBatches(listing, 3, (128, 96), seed=4).decoded_bytes()
    partial = 3 * 32400                                                            # the (90, 120) source, or a few smaller ones
    for kw in (dict(), dict(workers=4), dict(cache_bytes=full), dict(cache_bytes=partial), dict(cache_bytes=full, workers=4, prefetch=1)):
        reads.clear()
        before = jpeg.counters["calls"]
        loader, got = epochs(listing, 2, decode="gpu", **kw)
        for e in range(2):
            assert same(got[e], base[e]), (kw, e)
        calls = jpeg.counters["calls"] - before
        if kw.get("cache_bytes") == full:
            assert loader.resident_images() == 8 and len(reads) == 1 and calls == 3      # the second epoch decodes nothing
        elif kw.get("cache_bytes"):
            assert 0 < loader.resident_images() < 8 and 3 < calls <= 9      # a batch that straddles the arena's end takes two
        else:
            assert len(reads) == 2 and calls == 6                                   # PIL only ever sees the progressive file
    with pytest.raises(ValueError):
        aug.TrainBatches(listing, 3, (128, 96), seed=4, decode="cv2")


def test_resume_lands_on_the_same_batch(listing):
    kw = dict(multiscale=(64, 128), dim_interval=2, jitter=0.2)
    ref = aug.TrainBatches(listing, 2, (128, 96), seed=8, **kw)
    for _ in ref:
        pass
    want = [(x.cpu().numpy(), t.cpu().numpy()) for x, t in ref]                    # epoch 1 with decode="pil"
    loader = aug.TrainBatches(listing, 2, (128, 96), seed=8, decode="gpu", cache_bytes=1 << 20, **kw)
    for _ in loader:
        pass
    it = iter(loader)
    first = [next(it), next(it)]
    state = loader.state_dict()
    assert (state["epoch"], state["batch"]) == (1, 2)                             # the batch handed out, not the one decoding ahead
    assert "decode" not in state["config"]
    rest = [(x.cpu().numpy(), t.cpu().numpy()) for x, t in it]
    assert same([(x.cpu().numpy(), t.cpu().numpy()) for x, t in first] + rest, want)
    fresh = aug.TrainBatches(listing, 2, (128, 96), seed=8, decode="gpu", **kw)
    fresh.load_state_dict(state)
    assert same([(x.cpu().numpy(), t.cpu().numpy()) for x, t in fresh], want[2:])
    pil = aug.TrainBatches(listing, 2, (128, 96), seed=8, **kw)                    # the state of one setting resumes the other
    pil.load_state_dict(state)
    assert same([(x.cpu().numpy(), t.cpu().numpy()) for x, t in pil], want[2:])


def test_results_file_is_the_same(listing, tmp_path):
    # SW-1 weights with head biases at which a 96x96 input leaves some, not all, of its 567 rows above the evaluation threshold 0.005
    net = load_sw1_net(synth.weight_stream(b_obj=-1.0, b_cls=-4.0), size=96).cuda()
    names = ["c%d" % i for i in range(80)]
    outs = []
    for decode in ("pil", "gpu"):
        out = tmp_path / ("results_%s.json" % decode)
        n = evaluate.generate_results_file(net, listing, names, str(out), 3, (96, 96), is_letterbox=True, decode=decode)
        outs.append((n, out.read_bytes()))
    assert outs[0] == outs[1] and outs[0][0] > 0
