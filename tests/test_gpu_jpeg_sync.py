"""The self-synchronising entropy stage on the GPU (``yv3_jpeg_decode_batch_ex`` with ``YV3_JPEG_ENTROPY_PARALLEL``): one mixed batch of
every setting, scans longer than one window, the files of tests/jpeg_sync_cases.py for the workgroup logic (rounds of units, window
edges, cuts, the DC pass), damaged files whose status must be the serial stage's, and the Python surface."""
import io

import numpy as np
import pytest
import torch

from tests import jpeg_abi, jpeg_craft, jpeg_sync_cases
from tests.test_gpu_jpeg import damaged_files, files, lying_records, pil_rgb  # noqa: F401  (files: the fixture of every PIL setting)
from tests.test_jpeg_host import picture
from tests.test_jpeg_sync_host import crafted_long_files, table_files
from yolo_v3_amd import _ffi, evaluate, jpeg
from yolo_v3_amd import augment as aug

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SERIAL, PARALLEL = jpeg_abi.SERIAL, jpeg_abi.PARALLEL


def run_batch(datas, entropy, handed_null=False):
    """One yv3_jpeg_decode_batch_ex over ``datas`` through `tests.jpeg_abi.decode`, which asserts that nothing outside the
    destinations, the statuses, the counts and the workspace was written.  Returns statuses, hand-over counts and the destination
    bytes of every image.  ``handed_null``: the call gets no array for the counts (and those returned are the fill value)."""
    r = jpeg_abi.decode(datas, entry="ex", entropy=entropy, handed_null=handed_null)
    return r.statuses, r.handed, r.images


def test_every_setting_in_one_mixed_batch(files):
    cases, refs = files
    extra = table_files() + crafted_long_files()
    names = [n for n, _ in cases] + [n for n, _ in extra] + ["photograph again", "noise q100 4:4:4 again"]
    datas = [d for _, d in cases] + [d for _, d in extra] + [extra[0][1], extra[4][1]]       # windows: the same long files twice
    refs = list(refs) + [pil_rgb(d) for d in datas[len(cases):]]
    st1, ho1, px1 = run_batch(datas, PARALLEL)
    bad = [(names[k], int(st1[k]), int(ho1[k])) for k in range(len(datas)) if st1[k] or ho1[k]]
    assert not bad, bad[:10]                                             # status 0 and no unit handed over, for every file
    wrong = [names[k] for k in range(len(datas)) if not np.array_equal(px1[k], refs[k])]
    assert not wrong, (len(wrong), wrong[:10])                           # PIL's pixels, bit for bit
    st0, _, px0 = run_batch(datas, SERIAL)
    assert np.array_equal(st0, st1) and all(np.array_equal(a, b) for a, b in zip(px0, px1))
    st2, ho2, px2 = run_batch(datas, PARALLEL)                           # identical calls, identical bits
    assert np.array_equal(st2, st1) and np.array_equal(ho2, ho1) and all(np.array_equal(a, b) for a, b in zip(px2, px1))
    # both kinds of unit were met: scans of more than one window, units of one lane, and one image with both
    long_bytes = [len(d) for d in datas[len(cases):]]
    assert max(long_bytes) > 2 * 256 * 64 and min(len(d) for d in datas) < 700


# ---- the workgroup logic: tests/jpeg_sync_cases.py has the table of which file reaches which path, and test_jpeg_sync_host asserts
# on the CPU that each file is what its name says ---------------------------------------------------------------------------------
def check_good_files(files):
    """PARALLEL, SERIAL and PARALLEL again over one batch of valid files: status 0 and nothing handed over, PIL's pixels, the
    serial stage's, and the same bytes from the same call."""
    names, datas = [n for n, _ in files], [d for _, d in files]
    refs = [pil_rgb(d) for d in datas]
    st1, ho1, px1 = run_batch(datas, PARALLEL)
    bad = [(names[k], int(st1[k]), int(ho1[k])) for k in range(len(datas)) if st1[k] or ho1[k]]
    assert not bad, bad[:10]
    wrong = [names[k] for k in range(len(datas)) if not np.array_equal(px1[k], refs[k])]
    assert not wrong, (len(wrong), wrong[:10])
    st0, _, px0 = run_batch(datas, SERIAL)
    assert np.array_equal(st0, st1)
    wrong = [names[k] for k in range(len(datas)) if not np.array_equal(px1[k], px0[k])]
    assert not wrong, (len(wrong), wrong[:10])
    st2, ho2, px2 = run_batch(datas, PARALLEL)
    assert np.array_equal(st2, st1) and np.array_equal(ho2, ho1)
    wrong = [names[k] for k in range(len(datas)) if not np.array_equal(px2[k], px1[k])]
    assert not wrong, (len(wrong), wrong[:10])


def test_unit_rounds():
    check_good_files(jpeg_sync_cases.rounds())


def test_window_edges():
    check_good_files(jpeg_sync_cases.window_edges())


def test_cuts():
    check_good_files(jpeg_sync_cases.cuts())


def test_dc_shapes():
    check_good_files(jpeg_sync_cases.dc_shapes())


def test_batch_positions_do_not_interact():
    """Many rounds of long units, one short unit, one exactly full window and a unit handed over in round two, side by side in
    two orders: no workgroup's outcome depends on where its image stands in the batch."""
    files = [dict(jpeg_sync_cases.rounds())["4:2:0 512 long units"], table_files()[5][1],
             dict(jpeg_sync_cases.window_edges())["grey noise nsub 256"], jpeg_sync_cases.damaged_round_two()[1]]
    refs = [pil_rgb(d) for d in files[:3]]
    st0, _, _ = run_batch(files, SERIAL)
    assert list(st0[:3]) == [0, 0, 0] and st0[3] != 0
    seen = []
    for order in ([0, 1, 2, 3], [3, 2, 0, 1]):
        st, ho, px = run_batch([files[j] for j in order], PARALLEL)
        by_file = {j: (int(st[k]), int(ho[k])) for k, j in enumerate(order)}
        assert [by_file[j] for j in range(3)] == [(0, 0)] * 3, (order, by_file)
        assert by_file[3][0] == st0[3] and by_file[3][1] >= 1, (order, by_file)
        for k, j in enumerate(order):
            if j < 3:
                assert np.array_equal(px[k], refs[j]), (order, j)
        seen.append(by_file)
    assert seen[0] == seen[1]


def test_null_handed_over():
    """No array for the hand-over counts: the same statuses and bytes, for valid files of every kind of round and for one whose
    round two hands a unit over."""
    datas = [d for _, d in jpeg_sync_cases.rounds()] + [jpeg_sync_cases.damaged_round_two()[1]]
    st1, ho1, px1 = run_batch(datas, PARALLEL)
    assert list(ho1[:-1]) == [0] * (len(datas) - 1) and ho1[-1] >= 1 and list(st1[:-1]) == [0] * (len(datas) - 1) and st1[-1] != 0
    st2, _, px2 = run_batch(datas, PARALLEL, handed_null=True)
    assert np.array_equal(st1, st2) and all(np.array_equal(a, b) for a, b in zip(px1, px2))


# (file of rounds(), seed of `jpeg_craft.corruptions`, files at status 0, files at another status): three quarters of what the
# serial routine gives for the 150 files of each seed, which is 21 and 129 for the 512-unit file, 20 and 130 for the striped one
DAMAGE = [("4:2:0 512 long units", 11, 15, 96), ("4:2:0 stripes", 12, 15, 97)]


def test_damage_inside_long_restart_units():
    """One byte of the scan replaced, in files whose every (or every other) restart unit is long: the status is the serial
    stage's, and where it is 0 so are the pixels, and PIL's where PIL takes the file.

    Whether a unit can be handed over and yet decode (status 0, the only case in which the re-zeroed, serially decoded unit
    shows in the pixels) was searched for with the host program over these two sets and ten more seeds of each file (100 to
    109 and 200 to 209): among 3275 parser-accepted files, 2823 handed a unit over and none of those had status 0."""
    files = dict(jpeg_sync_cases.rounds())
    datas, groups = [], []
    for name, seed, _, _ in DAMAGE:
        group = [d for d in jpeg_craft.corruptions(files[name], 150, seed) if jpeg.parse(d).reason == 0]
        groups.append(range(len(datas), len(datas) + len(group)))
        datas += group
    st0, _, px0 = run_batch(datas, SERIAL)
    st1, ho1, px1 = run_batch(datas, PARALLEL)
    for (name, seed, ok, err), group in zip(DAMAGE, groups):
        n_ok, n_err = int((st0[group] == 0).sum()), int((st0[group] != 0).sum())
        print("%s seed %d: serial status 0 for %d files, another for %d; units handed over by the parallel stage in %d files"
              % (name, seed, n_ok, n_err, int((ho1[group] > 0).sum())))
        assert n_ok >= ok and n_err >= err, (name, n_ok, n_err)
    assert np.array_equal(st0, st1), [(k, int(a), int(b)) for k, (a, b) in enumerate(zip(st0, st1)) if a != b][:10]
    unit_codes = (_ffi.JPEG_S_CODE, _ffi.JPEG_S_OVERRUN, _ffi.JPEG_S_COEF, _ffi.JPEG_S_EXTRA, _ffi.JPEG_S_DC)
    g = groups[0]                                                    # every unit long: such a status can only come from a handed-over unit
    assert (ho1[g][np.isin(st1[g], unit_codes)] >= 1).all() and np.isin(st1[g], unit_codes).sum() > 0
    for k, d in enumerate(datas):
        if st1[k] == 0:
            assert np.array_equal(px1[k], px0[k]), k
            try:
                ref = pil_rgb(d)
            except Exception:
                continue
            assert np.array_equal(px1[k], ref), k


def test_damaged_files_get_the_serial_status():
    good, truncated, corrupted = damaged_files()
    other = jpeg_craft.pil_bytes(np.asarray(picture(33, 19, seed=12)), quality=75, subsampling=1, restart_marker_blocks=2)
    lost_marker = other.replace(b"\xff\xd1", b"\x12\x34", 1)
    sources = jpeg_craft.corruption_sources()
    datas = [good, truncated, other, corrupted, lost_marker, good[:-2]]
    for (name, src), seed in list(zip(sources, jpeg_craft.CORRUPTION_SEEDS))[:2]:
        datas += jpeg_craft.corruptions(src, 300, seed)
    long_src = table_files()[1][1]                                       # damage inside a scan of several windows' worth of passes
    datas += jpeg_craft.corruptions(long_src, 40, 3)
    datas = [d for d in datas if jpeg.parse(d).reason == 0]
    assert len(datas) > 600
    st0, _, px0 = run_batch(datas, SERIAL)
    st1, ho1, px1 = run_batch(datas, PARALLEL)
    assert np.array_equal(st0, st1), [(k, int(a), int(b)) for k, (a, b) in enumerate(zip(st0, st1)) if a != b][:10]
    assert (st1 == 0).sum() > 30 and (st1 != 0).sum() > 100 and ho1.sum() > 0 and (ho1[st1 != 0] >= 0).all()
    for k, d in enumerate(datas):
        if st1[k] == 0:
            assert np.array_equal(px1[k], px0[k]), k
            try:
                ref = pil_rgb(d)
            except Exception:                                            # (a file without EOI: PIL refuses it, jpeg.py routes it)
                continue
            assert np.array_equal(px1[k], ref), k


def test_lying_records_stay_inside_their_buffers():
    """test_gpu_jpeg's lying-record case through the parallel stage: the same statuses as the serial one."""
    good, _, _ = damaged_files()
    results = [jpeg_abi.decode([good], entry="ex", entropy=entropy, order=[0, 0, 0, 0], dev_infos=lying_records(good), dst_cut=1)
               for entropy in (SERIAL, PARALLEL)]
    assert results[1].handed.tolist() == [0, 0, 0, 0]
    assert results[0].statuses.tolist() == results[1].statuses.tolist() == [0, _ffi.JPEG_S_BOUNDS, _ffi.JPEG_S_INFO, _ffi.JPEG_S_BOUNDS]
    assert all(np.array_equal(a, b) for a, b in zip(results[0].images, results[1].images))
    assert np.array_equal(results[1].images[0], pil_rgb(good)) and all((px == jpeg_abi.FILL).all() for px in results[1].images[1:])


def test_decode_batch_parallel_one_upload_one_status_read(files):
    cases, refs = files
    pick = list(range(0, len(cases), 37))
    photo = table_files()[0][1]
    before = dict(jpeg.counters)
    out = jpeg.decode_batch([cases[j][1] for j in pick] + [photo], device=DEV, entropy="parallel")
    assert {k: jpeg.counters[k] - before[k] for k in ("calls", "uploads", "status_reads", "fallbacks")} == \
        {"calls": 1, "uploads": 1, "status_reads": 1, "fallbacks": 0}
    assert out.fallback == [False] * (len(pick) + 1) and out.handed_over == [0] * (len(pick) + 1)
    for t, j in zip(out, pick):
        assert np.array_equal(t.cpu().numpy(), refs[j]), cases[j][0]
    assert np.array_equal(out[-1].cpu().numpy(), pil_rgb(photo))
    again = jpeg.decode_batch([cases[j][1] for j in pick] + [photo], device=DEV, entropy="parallel")
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    assert jpeg.decode_batch([photo], device=DEV).handed_over == [0]     # the serial stage: zeros


def test_damaged_files_come_back_through_pil_with_parallel():
    good, truncated, corrupted = damaged_files()
    progressive = jpeg_craft.pil_bytes(np.asarray(picture(17, 13, seed=13)), progressive=True)
    batch = [good, truncated, corrupted, progressive, good]
    out = jpeg.decode_batch(batch, device=DEV, errors="keep", entropy="parallel")
    ser = jpeg.decode_batch(batch, device=DEV, errors="keep")
    assert out.fallback == ser.fallback == [False, True, True, True, False] and out.reasons == ser.reasons
    assert out.reasons[2] == ("device", _ffi.JPEG_S_CODE) and out.reasons[3] == ("parser", _ffi.JPEG_PROGRESSIVE)
    assert out.handed_over[0] == 0 and out.handed_over[1] >= 1 and out.handed_over[2] >= 1 and out.handed_over[3] == 0
    for i, data in enumerate(batch):
        try:
            ref = evaluate.read_image_rgb(io.BytesIO(data))
        except Exception as e:
            assert type(out[i]) is type(e) and str(out[i]) == str(e) and i == 1
            continue
        assert np.array_equal(out[i].cpu().numpy(), ref), i


def test_train_batches_with_the_parallel_stage(tmp_path):
    (tmp_path / "images").mkdir()
    (tmp_path / "labels").mkdir()
    paths = []
    for i, ((w, h), kw) in enumerate([((120, 90), dict(subsampling=2)), ((70, 90), dict(subsampling=1, restart_marker_blocks=3)),
                                      ((64, 64), dict(subsampling=0)), ((57, 31), dict())]):
        p = str(tmp_path / "images" / ("img%d.jpg" % i))
        picture(w, h, "L" if i == 3 else "RGB", "gradient" if i % 2 else "noise", seed=60 + i).save(p, "JPEG", quality=85, **kw)
        np.savetxt(str(tmp_path / "labels" / ("img%d.txt" % i)), np.array([[1, 0.5, 0.5, 0.3, 0.4]]))
        paths.append(p)
    lst = tmp_path / "train.txt"
    lst.write_text("\n".join(paths) + "\n")

    def epoch(**kw):
        return [(x.cpu().numpy(), t.cpu().numpy()) for x, t in aug.TrainBatches(str(lst), 2, (128, 96), seed=4, jitter=0.2, **kw)]
    base = epoch()
    got = epoch(decode="gpu", entropy="parallel")
    assert len(base) == len(got) == 2
    for (x, t), (x0, t0) in zip(got, base):
        assert np.array_equal(x.view(np.int32), x0.view(np.int32)) and np.array_equal(t.view(np.int32), t0.view(np.int32))
    with pytest.raises(ValueError):
        aug.TrainBatches(str(lst), 2, (128, 96), seed=4, decode="gpu", entropy="fast")
