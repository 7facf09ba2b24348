"""Progressive JPEG decode on the GPU (entropy_prog_kernel of csrc/jpeg.hip through ``yolo_v3_amd.jpeg`` with
``progressive=True``) against PIL's decode of the same bytes, bit for bit: the PIL-written and crafted files of
`tests.jpeg_prog_craft` in batches of 16 that mix them with baseline, refused, EXIF-rotated, truncated and corrupted files; the
device's status of damaged files against the stand-alone host program's; the launch count without a progressive file; the
parallel entropy stage, determinism, the ``dst=`` arena and the workspace's bounds; and the switch in `TrainBatches` and
`generate_results_file`."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_abi
from tests import jpeg_prog_craft as craft
from tests.helpers import load_sw1_net
from tests.test_gpu_jpeg_loader import epochs, listing, same          # noqa: F401  (listing: a fixture)
from tests.test_jpeg_prog_host import build_checker, host_decode
from yolo_v3_amd import _ffi, evaluate, jpeg, synth
from yolo_v3_amd import augment as aug

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def reference(data):
    """`read_image_rgb`'s pixels of ``data``, or the exception it raises."""
    try:
        return evaluate.read_image_rgb(io.BytesIO(data))
    except Exception as e:
        return e


def check_against_pil(out, batch, names):
    for i, data in enumerate(batch):
        ref = reference(data)
        if isinstance(ref, Exception):
            assert type(out[i]) is type(ref) and str(out[i]) == str(ref), names[i]
            assert out.fallback[i], names[i]
        else:
            assert torch.is_tensor(out[i]) and np.array_equal(out[i].cpu().numpy(), ref), names[i]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/jpeg_prog_host_check.cpp as a plain program, WITHOUT sanitizers: here it only supplies the host routine's statuses.
    (The sanitizer build of the same source belongs to the CPU tests of tests/test_jpeg_prog_host.py.)"""
    return build_checker(tmp_path_factory.mktemp("jpeg_prog_plain") / "jpeg_prog_host_check", sanitize=False)


@pytest.fixture(scope="module")
def extras():
    """The files mixed into every batch: (name, bytes, the first word of the expected reason or None)."""
    prog = craft.valid_files()[3 * 18 * 7 + 5 * 18 + 6][1]              # a 4:2:0 40x24 file
    info, rec = jpeg.parse_ex(prog)
    assert rec is not None and (info.width, info.height) == (40, 24)
    exif = Image.Exif()
    exif[0x0112] = 6
    b = io.BytesIO()
    Image.fromarray(np.random.RandomState(3).randint(0, 256, (24, 40, 3)).astype(np.uint8)).save(b, "JPEG", progressive=True, exif=exif)
    first = rec.scans[0]
    mid = int(first.offset + first.length // 2)
    return [("exif-rotated", b.getvalue(), "exif"), ("truncated", prog[:-12], "device"),
            ("corrupted", prog[:mid] + b"\xff\x00" * 4 + prog[mid + 8:], "device")]


def test_valid_and_crafted_files_in_mixed_batches(extras):
    """Batches of 16: eleven progressive files, a baseline twin, a refused script and the three extras.  Every image is PIL's,
    and `fallback` / `reasons` say which way each went.  Images are at most 96x80 with two exceptions among the crafted files,
    whose cases need the size: "eob14 across block rows" (1032x1024: an EOB run of 16384 blocks or more needs that many blocks)
    and "more units than lanes" (160x120: 300 blocks, one per unit, for more than 256 units in one level)."""
    family = craft.valid_files() + craft.crafted()
    refused = craft.refused_scripts()
    assert jpeg.Source(extras[1][1], progressive=True).on_gpu and jpeg.Source(extras[2][1], progressive=True).on_gpu
    for n, start in enumerate(range(0, len(family), 11)):
        part = family[start:start + 11]
        rname, rdata, rreason = refused[n % len(refused)]
        batch = [f for _, f, _ in part] + [part[0][2], rdata] + [e[1] for e in extras]
        names = [name for name, _, _ in part] + ["twin of " + part[0][0], rname] + [e[0] for e in extras]
        before = dict(jpeg.counters)
        out = jpeg.decode_batch(batch, device=DEV, errors="keep", progressive=True)
        assert {k: jpeg.counters[k] - before[k] for k in ("calls", "uploads", "status_reads", "launches", "prog_images")} == \
            {"calls": 1, "uploads": 1, "status_reads": 1, "launches": 5, "prog_images": len(part) + 2}
        k = len(part)
        assert out.fallback == [False] * (k + 1) + [True] * 4, names
        assert out.reasons[:k + 1] == [None] * (k + 1)
        assert out.reasons[k + 1] == ("parser", getattr(_ffi, rreason))
        assert out.reasons[k + 2] == ("exif", None)
        assert out.reasons[k + 3][0] == "device" and out.reasons[k + 3][1] != 0
        assert out.reasons[k + 4][0] == "device" and out.reasons[k + 4][1] != 0
        check_against_pil(out, batch, names)


def test_device_status_equals_the_host_programs(checker, tmp_path):
    """A fixed seeded list of damaged files: the status the device reports is the host program's (which runs the same routine
    level by level); status 0 means PIL's pixels."""
    files = []
    for (name, data), seed in zip(craft.damage_sources(), craft.DAMAGE_SEEDS):
        files += craft.corruptions(data, 48, seed + 100)
        first, last = craft.scan_data_range(data)
        files += [data[:cut] for cut in range(last - 1, first, -max(1, (last - first) // 12))][:12]
    host = host_decode(checker, tmp_path, files)
    on_device = [(f, h) for f, h in zip(files, host) if h[1]]           # accepted by the parser
    assert len(on_device) >= 100
    seen = set()
    for start in range(0, len(on_device), 16):
        part = on_device[start:start + 16]
        out = jpeg.decode_batch([f for f, _ in part], device=DEV, errors="keep", progressive=True)
        for i, (f, (reason, accepted, status, _, px)) in enumerate(part):
            r = out.reasons[i]
            assert r is None or r[0] in ("device", "truncated"), r
            device = r[1] if r is not None and r[0] == "device" else 0
            assert device == status, (start + i, device, status)
            seen.add(status)
            if status == 0 and r is None:
                assert np.array_equal(out[i].cpu().numpy(), px) and np.array_equal(px, craft.pil_pixels(f))
        check_against_pil(out, [f for f, _ in part], list(range(start, start + len(part))))
    assert 0 in seen and len(seen) >= 4


def test_a_batch_without_a_progressive_file_takes_the_old_call(extras):
    """`jpeg.counters["launches"]` is the library's own count of the kernels it launched (yv3_jpeg_launch_count), read around the
    call: four without a progressive image, whatever the switch says.  (yv3_jpeg_decode_batch_prog itself with P = 0:
    `test_the_workspace_stays_between_its_sentinels`.)"""
    baseline = [t for _, _, t in craft.valid_files()[::63]]
    refs = [craft.pil_pixels(t) for t in baseline]
    before = dict(jpeg.counters)
    out = jpeg.decode_batch(baseline, device=DEV, progressive=True)
    assert jpeg.counters["launches"] - before["launches"] == 4 and jpeg.counters["prog_images"] == before["prog_images"]
    uploaded = jpeg.counters["upload_bytes"] - before["upload_bytes"]
    again = jpeg.decode_batch(baseline, device=DEV)                    # the switch off: the same upload, byte for byte in size
    assert jpeg.counters["upload_bytes"] - before["upload_bytes"] == 2 * uploaded
    for a, b, r in zip(out, again, refs):
        assert np.array_equal(a.cpu().numpy(), r) and np.array_equal(b.cpu().numpy(), r)
    # with the switch off a progressive file is refused as before and read by PIL once
    prog = craft.valid_files()[100][1]
    before = dict(jpeg.counters)
    out = jpeg.decode_batch([prog, baseline[0]], device=DEV)
    assert out.reasons == [("parser", _ffi.JPEG_PROGRESSIVE), None] and out.fallback == [True, False]
    assert jpeg.counters["fallbacks"] - before["fallbacks"] == 1 and jpeg.counters["launches"] - before["launches"] == 4
    assert np.array_equal(out[0].cpu().numpy(), craft.pil_pixels(prog))


def mixed_batch(extras):
    family = craft.valid_files()
    picks = [family[i] for i in (17, 95, 200, 333, 420, 503)] + craft.crafted()[:5]
    batch = [f for _, f, _ in picks] + [picks[1][2], picks[4][2]] + [extras[1][1], extras[2][1]]
    restarts = jpeg_restart_twin()
    return batch + [restarts]


def jpeg_restart_twin():
    """A baseline file with a scan long enough for the parallel entropy stage."""
    a = np.random.RandomState(8).randint(0, 256, (80, 96, 3)).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=95, subsampling=0)
    return b.getvalue()


def test_parallel_entropy_and_repeated_calls_give_the_same(extras):
    batch = mixed_batch(extras)
    serial = jpeg.decode_batch(batch, device=DEV, errors="keep", progressive=True)
    again = jpeg.decode_batch(batch, device=DEV, errors="keep", progressive=True)
    parallel = jpeg.decode_batch(batch, device=DEV, errors="keep", progressive=True, entropy="parallel")
    assert serial.reasons == again.reasons == parallel.reasons and serial.fallback == parallel.fallback
    assert serial.fallback == [False] * 13 + [True, True, False]
    assert parallel.handed_over == [0] * len(batch)
    for i in range(len(batch)):
        if torch.is_tensor(serial[i]):
            a = serial[i].cpu().numpy()
            assert np.array_equal(a, again[i].cpu().numpy()) and np.array_equal(a, parallel[i].cpu().numpy()), i
    check_against_pil(serial, batch, list(range(len(batch))))


def test_the_dst_arena_path(extras):
    family = craft.valid_files()
    batch = [family[i][1] for i in (30, 250, 480)] + [family[30][2], craft.refused_scripts()[0][1], craft.crafted()[2][1]]
    refs = [craft.pil_pixels(d) for d in batch]
    offsets, pos = [], 7
    for r in refs:
        offsets.append(pos)
        pos += r.size + 13
    arena = torch.full((pos,), 0xA5, dtype=torch.uint8, device=DEV)
    out = jpeg.submit(batch, device=DEV, dst=(arena, offsets), progressive=True).finish()
    assert out.fallback == [False, False, False, False, True, False]
    got = arena.cpu().numpy()
    mask = np.ones(got.size, bool)
    for t, r, o in zip(out, refs, offsets):
        assert t.data_ptr() == arena.data_ptr() + o
        assert np.array_equal(got[o:o + r.size].reshape(r.shape), r)
        mask[o:o + r.size] = False
    assert (got[mask] == 0xA5).all()


def test_the_workspace_stays_between_its_sentinels():
    """One yv3_jpeg_decode_batch_prog through the C ABI: progressive and baseline images, a workspace of exactly the queried
    size between guard bytes, destinations between guard bytes, and a device record that lies about a scan's range."""
    family = craft.valid_files()
    picks = [family[i] for i in (5, 77, 150, 260, 371, 499)] + craft.crafted()[:5] + [craft.crafted()[7]]
    datas = [f for _, f, _ in picks] + [picks[0][2], picks[3][2]] + [picks[2][1]]
    B = len(datas)
    progs = [rec for rec in (jpeg.parse_ex(d)[1] for d in datas) if rec is not None]
    P = len(progs)
    assert P == B - 2
    prog_dev = (_ffi.JpegProg * P)(*progs)
    prog_dev[P - 1].scans[2].length = 1 << 30                           # the last image's DEVICE record lies: past the source buffer
    refs = [craft.pil_pixels(d) for d in datas]
    r = jpeg_abi.decode(datas, entry="prog", dev_progs=prog_dev)
    assert r.launches == 5
    assert r.statuses.tolist() == [0] * (B - 1) + [_ffi.JPEG_S_BOUNDS]
    for k in range(B - 1):
        assert np.array_equal(r.images[k], refs[k]), k
    assert (r.images[B - 1] == jpeg_abi.FILL).all()                     # the refused image's destination too
    # the same entry with P = 0 over the two baseline images of the batch: four launches, no entropy_prog_kernel
    k0 = B - 3
    r0 = jpeg_abi.decode(datas[k0:k0 + 2], entry="prog")
    assert 0 < r0.need <= r.need and r0.launches == 4
    assert r0.statuses.tolist() == [0, 0]
    assert np.array_equal(r0.images[0], refs[k0]) and np.array_equal(r0.images[1], refs[k0 + 1])      # the same pixels again


def test_train_batches_and_the_results_file_with_the_switch(listing, monkeypatch, tmp_path):
    """The list of `tests.test_gpu_jpeg_loader` holds one progressive file: with ``progressive=True`` PIL never sees it, with the
    switch off it is refused with JPEG_PROGRESSIVE and read by PIL as before; the batches and the results file are the same."""
    _, base = epochs(listing, 1)                                        # decode="pil"
    reads = []
    real = evaluate.read_image_rgb

    def counting_read(path):
        reads.append(path)
        return real(path)
    monkeypatch.setattr(evaluate, "read_image_rgb", counting_read)
    full = aug.TrainBatches(listing, 3, (128, 96), seed=4).decoded_bytes()
    for kw in (dict(), dict(workers=2), dict(cache_bytes=full)):
        reads.clear()
        before = dict(jpeg.counters)
        _, got = epochs(listing, 1, decode="gpu", progressive=True, **kw)
        assert same(got[0], base[0]), kw
        assert reads == [] and jpeg.counters["fallbacks"] == before["fallbacks"], kw
        assert jpeg.counters["prog_images"] - before["prog_images"] == 1
    reads.clear()
    loader, got = epochs(listing, 1, decode="gpu")
    assert same(got[0], base[0]) and len(reads) == 1 and not loader.progressive
    assert "progressive" not in loader.state_dict()["config"]
    assert "progressive" not in aug.TrainBatches(listing, 3, (128, 96), seed=4, decode="gpu", progressive=True).state_dict()["config"]
    paths = open(listing).read().split()
    src = jpeg.Source(paths[6])
    assert not src.on_gpu and src.info.reason == _ffi.JPEG_PROGRESSIVE
    net = load_sw1_net(synth.weight_stream(b_obj=-1.0, b_cls=-4.0), size=96).cuda()
    names = ["c%d" % i for i in range(80)]
    outs = []
    for kw in (dict(decode="pil"), dict(decode="gpu", progressive=True), dict(decode="gpu")):
        reads.clear()
        out = tmp_path / ("results_%d.json" % len(outs))
        n = evaluate.generate_results_file(net, listing, names, str(out), 3, (96, 96), is_letterbox=True, **kw)
        outs.append((n, out.read_bytes()))
        if kw["decode"] == "gpu":
            assert len(reads) == (0 if kw.get("progressive") else 1), kw
    assert outs[0] == outs[1] == outs[2] and outs[0][0] > 0
