"""ExtraAugmentations without a GPU: the numpy restatement tests/extra_aug_ref.py against scipy (the two blurs the reference
reaches scipy for) and against values worked by hand, the Philox / Box-Muller generator, the host's draws and checks
(yolo_v3_amd/extra_augment.py) and the C interface's declarations."""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import extra_aug_ref as R
from yolo_v3_amd import _ffi
from yolo_v3_amd import augment as aug
from yolo_v3_amd import extra_augment as extra

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS, MEDIANS = (0.05, 0.13, 0.7, 1.5, 3.0), (3, 5, 7, 9, 11)


def planes():
    """Random planes, constant planes and planes shorter than every radius."""
    rng = np.random.RandomState(7)
    out = [rng.randint(0, 256, s).astype(np.uint8) for s in [(1, 1), (1, 7), (5, 3), (13, 9), (33, 47), (60, 41)]]
    out += [np.full(s, v, dtype=np.uint8) for s in [(1, 1), (1, 7), (5, 3), (13, 9), (40, 40)] for v in (0, 1, 127, 200, 255)]
    return out


def test_gauss_and_median_equal_scipy_bit_for_bit():
    ndimage = pytest.importorskip("scipy.ndimage")
    changed = False
    for a in planes():
        for sigma in SIGMAS:
            want = ndimage.gaussian_filter(a, sigma)
            assert np.array_equal(R.gauss(a, sigma), want), (a.shape, sigma)
            changed |= a.min() == a.max() and not np.array_equal(want, a)
        for k in MEDIANS:
            assert np.array_equal(R.median(a, k), ndimage.median_filter(a, size=k, mode="nearest")), (a.shape, k)
    assert changed                                          # a constant plane does come out one lower: the truncations matter
    assert R.gauss_radius(0.05) == 0 and R.gauss_radius(3.0) == 12
    assert np.array_equal(extra.gauss_weights(1.3), R.gauss_weights(1.3)) and extra.gauss_radius(0.13) == 1


def test_philox_known_answer_and_box_muller_moments():
    # Random123's kat_vectors: philox4x32-10 of counter 0, key 0.  The restatement follows the published algorithm (Salmon et
    # al. 2011, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl 0x9E3779B9 / 0xBB67AE85) and agrees with the vector as recalled.
    x = R.philox4x32(np.zeros((1, 4), np.uint32), np.zeros((1, 2), np.uint32))[0]
    assert [int(v) for v in x] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    a = R.philox4x32(np.array([[1, 2, 0, 0]], np.uint32), np.array([[3, 4]], np.uint32))[0]
    assert not np.array_equal(a, x)
    n = 10 ** 5
    z = R.normal(np.arange(n), 0x1234ABCD5678)
    assert abs(z.mean()) <= 4 / np.sqrt(n)                  # standard error of the mean of n unit normals
    assert abs(z.var() - 1) <= 4 * np.sqrt(2 / n)           # ... and of their variance
    assert np.array_equal(z[:50], R.normal(np.arange(50), 0x1234ABCD5678))
    hi = R.normal(np.array([2 ** 32 + 5], dtype=np.uint64), 9)                     # the counter's second word is the index's high half
    assert hi[0] != R.normal(np.array([5], dtype=np.uint64), 9)[0]


A3 = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], dtype=np.uint8)


def test_average_by_hand():
    # k = 3, reflect-101: the corner's window is rows (1, 0, 1) x columns (1, 0, 1) = 330 -> 36.67 -> 37
    assert R.average(A3, 3).tolist() == [[37, 40, 43], [47, 50, 53], [57, 60, 63]]
    # k = 2: the anchor is 1, so the window is (y - 1 .. y) x (x - 1 .. x); index -1 reflects to 1
    assert R.average(A3, 2).tolist() == [[30, 30, 40], [30, 30, 40], [60, 60, 70]]
    # 1 x 4: both rows of the window are row 0; 2 * (1 + 2) / 4 = 1.5 -> 2 and 2 * (2 + 3) / 4 = 2.5 -> 2: rint, half to even
    assert R.average(np.array([[1, 2, 3, 5]], dtype=np.uint8), 2).tolist() == [[2, 2, 2, 4]]
    assert R.average(np.array([[7]], dtype=np.uint8), 7).tolist() == [[7]]


def test_sharpen_by_hand():
    for img in (A3, np.array([[0, 255, 0, 255]], dtype=np.uint8)):
        assert np.array_equal(R.sharpen(img, 0.0, 1.5), img)                       # alpha = 0: the identity
    assert R.sharpen_kernel(0.5, 1.0).tolist() == [[-0.5, -0.5, -0.5], [-0.5, 5.0, -0.5], [-0.5, -0.5, -0.5]]
    assert R.sharpen_kernel(0.5, 1.0).dtype == np.float32
    # centre: 5 * 50 - 0.5 * 400 = 50; corner (0, 0): 5 * 10 - 0.5 * 320 = -110 -> 0; corner (2, 2): 5 * 90 - 0.5 * 480 = 210
    out = R.sharpen(A3, 0.5, 1.0)
    assert (out[1, 1], out[0, 0], out[2, 2]) == (50, 0, 210)
    # 1 x 4: at x = 1, 5 * 255 - 0.5 * 510 = 1020 -> 255; at x = 0 (columns 1, 0, 1), 0 - 0.5 * 1530 -> 0
    assert R.sharpen(np.array([[0, 255, 0, 255]], dtype=np.uint8), 0.5, 1.0).tolist() == [[0, 255, 0, 255]]


def test_add_mul_contrast_by_hand():
    img = np.zeros((1, 4, 3), dtype=np.uint8)
    img[0, :, :] = np.array([0, 3, 252, 255])[:, None]
    assert R.apply_step(img, ("ADD", 5, -5, 0))[0].T.tolist() == [[5, 8, 255, 255], [0, 0, 247, 250], [0, 3, 252, 255]]
    img[0, :, :] = np.array([0, 100, 200, 255])[:, None]
    assert R.apply_step(img, ("MUL", 0.8, 1.2, 1.0))[0].T.tolist() == [[0, 80, 160, 204], [0, 120, 240, 255], [0, 100, 200, 255]]
    assert R.apply_step(img, ("CONTRAST", 0.5, 2.0, 1.0))[0].T.tolist() == [[64, 114, 164, 191], [0, 72, 255, 255], [0, 100, 200, 255]]
    # float32, not float64: float32(0.7) * 10 rounds to 7.0 (in float64 it is 6.9999998 -> 6)
    ten = np.full((3, 3, 3), 10, dtype=np.uint8)
    assert R.apply_step(ten, ("MUL", 0.7, 0.7, 0.7)).tolist() == np.full((3, 3, 3), 7).tolist() and int(10 * float(np.float32(0.7))) == 6
    # scale 0 is the identity; a program runs its steps in order
    assert np.array_equal(R.apply_step(img, ("NOISE", 0.0, True, 5)), img)
    assert not R.noise_mask(img, 0.0, True, 5).any()
    two = R.extra_ref([img], [[("ADD", 5, 5, 5), ("MUL", 1.2, 1.2, 1.2)]])[0]
    assert two[0, :, 0].tolist() == [6, 126, 246, 255] and R.extra_ref([img], [[]])[0].tolist() == img.tolist()


def test_noise_moves_bytes_as_defined():
    img = np.full((40, 50, 3), 128, dtype=np.uint8)
    one = R.apply_step(img, ("NOISE", 12.75, False, 77)).astype(np.int32)
    three = R.apply_step(img, ("NOISE", 12.75, True, 77)).astype(np.int32)
    assert (one[:, :, 0] == one[:, :, 1]).all() and (one[:, :, 1] == one[:, :, 2]).all()           # one draw per pixel
    assert (three[:, :, 0] != three[:, :, 1]).any()
    z = R.normal(np.arange(2000, dtype=np.uint64), 77).reshape(40, 50)
    assert np.array_equal(one[:, :, 0], np.trunc(128 + 12.75 * z).astype(np.int32))
    z3 = R.normal(np.arange(6000, dtype=np.uint64), 77).reshape(40, 50, 3)                         # element (y W + x) 3 + c
    assert np.array_equal(three, np.trunc(128 + 12.75 * z3).astype(np.int32))
    assert abs(one.std() - 12.75) < 1.0
    dark = R.apply_step(np.zeros((8, 8, 3), np.uint8), ("NOISE", 12.75, True, 1))
    assert dark.min() == 0 and dark.max() > 0                                                      # clipped below, truncated above


# ---- the host's draws -------------------------------------------------------------------------------------------------------------
def test_sample_extra_is_a_function_of_the_seeds_and_leaves_sample_params_alone():
    seeds, shapes = [0, 1, 2 ** 31 - 2, 12345], [(480, 640), (1, 1), (33, 47), (5, 3)]
    before = aug.sample_params(seeds, shapes=shapes)
    a = extra.sample_extra(seeds, shapes)
    assert a == extra.sample_extra(seeds, shapes) and a == aug.sample_extra(seeds, [(9, 9)] * 4)
    assert np.array_equal(aug.sample_params(seeds, shapes=shapes), before)
    assert extra.sample_extra(seeds[:1], shapes[:1])[0] != extra.sample_extra([7], shapes[:1])[0]
    with pytest.raises(ValueError):
        extra.sample_extra(seeds, shapes[:2])


def test_sample_extra_ranges_and_frequencies():
    n = 2000
    programs = extra.sample_extra(range(n), [(4, 4)] * n)
    extra.check_programs(programs, [(4, 4)] * n)
    seen, single, orders = collections.Counter(), collections.Counter(), set()
    for prog in programs:
        ops = [s[0] for s in prog]
        assert 1 <= len(prog) <= 6 and len(set(ops)) == len(ops)
        assert sum(op in ("GAUSS", "AVERAGE", "MEDIAN") for op in ops) == 1                        # the blur group: exactly one
        orders.add(ops.index([op for op in ops if op in ("GAUSS", "AVERAGE", "MEDIAN")][0]))
        for s in prog:
            op, a = s[0], s[1:]
            seen[op] += 1
            if op == "GAUSS":
                assert 0.0 <= a[0] < 3.0
            elif op == "AVERAGE":
                assert isinstance(a[0], int) and 2 <= a[0] <= 7
            elif op == "MEDIAN":
                assert isinstance(a[0], int) and a[0] in (3, 5, 7, 9, 11)
            elif op == "SHARPEN":
                assert 0.0 <= a[0] < 0.5 and 0.75 <= a[1] < 1.5
            elif op == "NOISE":
                assert 0.0 <= a[0] < 0.05 * 255 and isinstance(a[1], bool) and 0 <= a[2] < 2 ** 64
                single["NOISE"] += not a[1]
            else:
                lo, hi = {"ADD": (-5, 5), "MUL": (0.8, 1.2), "CONTRAST": (0.5, 2.0)}[op]
                assert all(lo <= v <= hi for v in a)
                assert op != "ADD" or all(isinstance(v, int) for v in a)
                single[op] += a[0] == a[1] == a[2]
    for op in ("SHARPEN", "NOISE", "ADD", "MUL", "CONTRAST"):
        assert 0.40 * n <= seen[op] <= 0.60 * n, (op, seen[op])
    for op in ("GAUSS", "AVERAGE", "MEDIAN"):
        assert 0.28 * n <= seen[op] <= 0.39 * n, (op, seen[op])
    for op in ("NOISE", "MUL", "CONTRAST"):                                                        # the per_channel coin
        assert 0.40 * seen[op] <= single[op] <= 0.60 * seen[op], (op, single[op], seen[op])
    assert orders == set(range(6))                                                                  # the blur lands in every position
    assert {s[1] for p in programs for s in p if s[0] == "MEDIAN"} == {3, 5, 7, 9, 11}
    assert {s[1] for p in programs for s in p if s[0] == "AVERAGE"} == {2, 3, 4, 5, 6, 7}
    assert {v for p in programs for s in p if s[0] == "ADD" for v in s[1:]} == set(range(-5, 6))


BAD_PROGRAMS = {
    "unknown operation": [("BLUR", 1.0)],
    "empty step": [()],
    "too many steps": [("ADD", 1, 1, 1)] * 7,
    "argument count": [("SHARPEN", 0.1)],
    "sigma < 0": [("GAUSS", -0.1)],
    "sigma nan": [("GAUSS", float("nan"))],
    "sigma inf": [("GAUSS", float("inf"))],
    "radius 13": [("GAUSS", 3.2)],
    "two tables": [("GAUSS", 1.0), ("GAUSS", 2.0)],
    "two sigmas of one radius": [("GAUSS", 1.0), ("GAUSS", 1.1)],
    "average 1": [("AVERAGE", 1)],
    "average 8": [("AVERAGE", 8)],
    "average 2.0": [("AVERAGE", 2.0)],
    "median 4": [("MEDIAN", 4)],
    "median 1": [("MEDIAN", 1)],
    "median 13": [("MEDIAN", 13)],
    "alpha nan": [("SHARPEN", float("nan"), 1.0)],
    "lightness inf": [("SHARPEN", 0.1, float("inf"))],
    "scale < 0": [("NOISE", -1.0, False, 1)],
    "scale inf": [("NOISE", float("inf"), False, 1)],
    "per_channel 2": [("NOISE", 1.0, 2, 1)],
    "key < 0": [("NOISE", 1.0, True, -1)],
    "key 2**64": [("NOISE", 1.0, True, 2 ** 64)],
    "add 0.5": [("ADD", 0.5, 0, 0)],
    "add 256": [("ADD", 0, 256, 0)],
    "mul nan": [("MUL", 1.0, float("nan"), 1.0)],
    "contrast inf": [("CONTRAST", 1.0, 1.0, float("inf"))],
}


@pytest.mark.parametrize("name", sorted(BAD_PROGRAMS))
def test_check_programs_raises(name):
    good = [("MEDIAN", 3), ("ADD", 1, 2, 3)]
    extra.check_programs([good, [], [("GAUSS", 1.0), ("GAUSS", 0.05), ("GAUSS", 1.0)]], [(4, 4)] * 3)   # radius 4, 0 and 4: one table
    with pytest.raises(_ffi.Yv3Error) as e:
        extra.check_programs([good, BAD_PROGRAMS[name]], [(4, 4), (4, 4)])
    assert e.value.code == _ffi.EINVAL and "image 1" in str(e.value)


def test_check_programs_shapes_and_counts():
    for shape in [(0, 4), (4, 0), (2 ** 28 + 1, 1)]:
        with pytest.raises(_ffi.Yv3Error):
            extra.check_programs([[]], [shape])
    with pytest.raises(ValueError):
        extra.check_programs([[]], [(4, 4), (4, 4)])


# ---- the C interface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_ffi_binds_the_entry_points():
    header = open(os.path.join(REPO, "include", "yv3.h")).read()
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("yv3_extra_augment_workspace_bytes", "yv3_extra_augment"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _ffi.EXPORTS and hasattr(handle, name)
    assert len(_ffi._SIGNATURES["yv3_extra_augment"][1]) == 13
    lib = _ffi.lib()
    assert lib.yv3_extra_augment_workspace_bytes(12345) == 12345 and lib.yv3_extra_augment_workspace_bytes(0) == 0
    assert lib.yv3_extra_augment(None, 1, None, None, None, 1, None, 1, None, None, 1, None, None) == _ffi.EINVAL   # before any launch
    for name, code in extra.OPS.items():
        assert int(re.search(r"YV3_EXTRA_%s\s*=\s*(\d+)" % name, header).group(1)) == code
    assert int(re.search(r"#define\s+YV3_EXTRA_MAX_STEPS\s+(\d+)", header).group(1)) == extra.MAX_STEPS
    assert int(re.search(r"#define\s+YV3_EXTRA_MAX_RADIUS\s+(\d+)", header).group(1)) == extra.MAX_RADIUS


def test_program_layout_matches_the_c_header(tmp_path):
    """yv3_extra_program / yv3_extra_step as numpy packs them == as a C compiler sees include/yv3.h."""
    fields = [("yv3_extra_program", extra.PROGRAM, ["n_steps", "gauss_radius", "steps", "gauss_w"]),
              ("yv3_extra_step", extra.STEP, ["op", "k", "per_channel", "reserved", "v", "key"])]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv3.h"\nint main(void){\n' + "".join(
        'printf("%%zu ", sizeof(%s));\n' % t + "".join('printf("%%zu ", offsetof(%s, %s));\n' % (t, f) for f in names)
        for t, _, names in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    nums = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, dt, names in fields:
        want += [dt.itemsize] + [dt.fields[f][1] for f in names]
    assert nums == want
    packed = extra.pack_programs([[("GAUSS", 1.0), ("NOISE", 2.5, True, 2 ** 63 + 5), ("MEDIAN", 7), ("ADD", -5, 0, 5)]])[0]
    assert packed["n_steps"] == 4 and packed["gauss_radius"] == 4 and packed["steps"]["op"].tolist() == [1, 5, 3, 6, 0, 0]
    assert np.array_equal(packed["gauss_w"][:9], R.gauss_weights(1.0)) and not packed["gauss_w"][9:].any()
    assert packed["steps"]["key"][1] == 2 ** 63 + 5 and packed["steps"]["per_channel"][1] == 1 and packed["steps"]["k"][2] == 7
    assert packed["steps"]["v"][3].tolist() == [-5.0, 0.0, 5.0]


def test_train_batches_extra_switch_on_the_host(tmp_path):
    """The switch's host side: programs are drawn per batch from the schedule's seeds, and the state dict's config changes only
    when the switch is on."""
    from PIL import Image
    (tmp_path / "images").mkdir()
    paths = []
    for i in range(5):
        p = str(tmp_path / "images" / ("a%d.jpg" % i))
        Image.fromarray(np.full((6 + i, 9, 3), 40 * i, dtype=np.uint8)).save(p, format="PNG")
        paths.append(p)
    lst = tmp_path / "train.txt"
    lst.write_text("\n".join(paths) + "\n")
    off, default, on = (aug.TrainBatches(str(lst), 2, (64, 64), seed=3, **kw) for kw in (dict(extra=False), {}, dict(extra=True)))
    assert off.state_dict() == default.state_dict() and "extra" not in off.state_dict()["config"]
    assert on.state_dict()["config"]["extra"] is True
    on.load_state_dict(on.state_dict())
    off.load_state_dict(default.state_dict())
    with pytest.raises(ValueError):
        off.load_state_dict(on.state_dict())
    with pytest.raises(ValueError):
        on.load_state_dict(off.state_dict())
    order, seeds, _ = aug.epoch_schedule(3, 0, 5, 2)
    batches = list(on._host_batches())
    plain = list(default._host_batches())
    assert [b[5] for b in plain] == [None] * 3
    for k, (b, b0) in enumerate(zip(batches, plain)):
        assert b[5] == extra.sample_extra(seeds[2 * k:2 * k + 2], [(1, 1)] * len(b[0]))
        assert np.array_equal(b[3], b0[3]) and b[0] == b0[0]                                       # the other draws do not move
    assert len(list(on.host_batches())[0]) == 4
