"""The affine augmentation without a GPU: the numpy restatement tests/affine_aug_ref.py against Pillow (pixels, bit for bit) and
against boxes worked by hand, the host's draws and checks (yolo_v3_amd/affine_augment.py) and the C interface's declarations."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import affine_aug_ref as R
from yolo_v3_amd import _ffi
from yolo_v3_amd import affine_augment as affine
from yolo_v3_amd import augment as aug

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pillow(img, prog):
    H, W = img.shape[:2]
    out = Image.fromarray(img).transform((W, H), Image.AFFINE, tuple(float(v) for v in prog["inv"]), resample=Image.BILINEAR,
                                         fillcolor=(128, 128, 128))
    return np.asarray(out)


def cases():
    """(image, program): the corner sizes under every kind of program, then random sizes up to about 70 x 90."""
    rng = np.random.RandomState(11)
    sizes = [(1, 1), (1, 7), (7, 1), (4, 64), (5, 65), (33, 65), (70, 90)] + [(int(rng.randint(2, 71)), int(rng.randint(2, 91)))
                                                                             for _ in range(12)]
    out = []
    for i, (h, w) in enumerate(sizes):
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        kinds = [dict(),                                                                              # the identity
                 dict(theta=math.radians(45), scale=0.5, shear=math.radians(20)),
                 dict(theta=math.radians(-45), scale=2.0, shear=math.radians(-20)),
                 dict(theta=math.radians(rng.uniform(-45, 45)), scale=rng.uniform(0.5, 2.0), shear=math.radians(rng.uniform(-20, 20)),
                      tx=rng.uniform(-0.2, 0.2), ty=rng.uniform(-0.2, 0.2)),
                 dict(theta=math.radians(rng.uniform(-10, 10)), tx=0.6, ty=-0.45),                    # partly out
                 dict(tx=0.5), dict(ty=-0.25, scale=1.0),                                             # whole-pixel and half-pixel shifts
                 dict(tx=2.0, ty=0.1), dict(theta=math.radians(30), tx=-3.0, ty=3.0)]                # wholly out
        out += [(img, R.program(h, w, **kw), kw) for kw in kinds]
    return out


def test_pixels_equal_pillow_bit_for_bit():
    total = 0
    for img, prog, kw in cases():
        got, want = R.warp_ref(img, prog), pillow(img, prog)
        assert np.array_equal(got, want), (img.shape, kw, int((got != want).sum()))
        total += got.size
        if not kw:
            assert np.array_equal(got, img)                                        # the identity returns the source
        if abs(kw.get("tx", 0)) >= 2:
            assert (got == 128).all()                                              # pushed wholly out: every byte is the pad
        elif kw.get("tx") == 0.6 and min(img.shape[:2]) > 4:
            assert (got == 128).any() and (got != 128).any()
    assert total > 150000


def test_an_inactive_program_copies_the_image():
    img, prog, _ = cases()[-6]
    off = dict(prog, active=0)
    assert np.array_equal(R.warp_ref(img, off), img) and not np.array_equal(R.warp_ref(img, prog), img)


def test_inverse_against_numpy():
    shapes = [(1, 1), (48, 64), (480, 640), (1000, 37)]
    programs = affine.sample_affine(range(40), [shapes[i % 4] for i in range(40)], rotate=(-45, 45), scale=(0.5, 2.0), shear=(-20, 20),
                                    translate=(-0.5, 0.5), p=1.0)
    for prog in programs:
        full = np.linalg.inv(np.vstack([prog["fwd"].reshape(2, 3), [0.0, 0.0, 1.0]]))[:2].reshape(-1)
        # float64, a handful of operations on values up to about 1e3: relative to the row's largest coefficient
        scale = np.repeat(np.abs(full.reshape(2, 3)).max(axis=1), 3)
        assert np.all(np.abs(prog["inv"] - full) <= 1e-12 * scale), (prog, full)
        ref_fwd, ref_inv = R.matrices(*prog["shape"], theta=math.radians(prog["rotate"]), scale=prog["scale"],
                                      shear=math.radians(prog["shear"]), tx=prog["tx"], ty=prog["ty"])
        assert np.allclose(prog["fwd"], ref_fwd, rtol=1e-12, atol=1e-9) and np.allclose(prog["inv"], ref_inv, rtol=1e-12, atol=1e-9)


# ---- labels --------------------------------------------------------------------------------------------------------------------------
def test_labels_identity_keeps_interior_boxes_and_clips_at_the_border():
    prog = R.program(100, 100)
    rows = np.array([[2, 0.4, 0.45, 0.2, 0.3], [1, 0.75, 0.5, 0.5, 0.2]])
    out = R.labels_ref(rows, 100, 100, prog)
    assert np.abs(out[0] - rows[0]).max() <= 1e-12
    # x 50 .. 100 on a 100-pixel image: x2 is clipped to 100 - eps
    assert out[1, 0] == 1 and abs(out[1, 3] - (50 - R.EPS) / 100) <= 1e-15 and abs(out[1, 1] - (50 + (50 - R.EPS) / 2) / 100) <= 1e-15
    assert out[1, 3] < 0.5
    assert R.EPS == 2.0 ** -23


def test_labels_quarter_turn():
    prog = R.program(100, 100, theta=math.radians(90))
    out = R.labels_ref([[7, 0.3, 0.2, 0.2, 0.1]], 100, 100, prog)
    assert np.abs(out[0] - [7, 0.8, 0.3, 0.1, 0.2]).max() <= 1e-12


def test_labels_moved_out_cut_out_threshold_and_empty_rows():
    out = R.labels_ref([[1, 0.5, 0.5, 0.2, 0.2]], 100, 100, R.program(100, 100, tx=1.5))
    assert not out.any()                                                           # wholly outside: a zero row
    # identity on 128 x 128 (every number dyadic): x -72 .. 8 of which 0 .. 8 remain, 8 / 80 = 0.1 exactly -> dropped;
    # x -72 .. 8.0625: 8.0625 / 80.0625 > 0.1 -> kept, clipped to 0 .. 8.0625
    prog = R.program(128, 128)
    assert prog["fwd"].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    at = [3, (-72 + 8) / 2 / 128, 0.5, 80 / 128, 0.25]
    above = [3, (-72 + 8.0625) / 2 / 128, 0.5, 80.0625 / 128, 0.25]
    out = R.labels_ref([at, above], 128, 128, prog)
    assert not out[0].any()
    assert out[1].tolist() == [3, 8.0625 / 2 / 128, 0.5, 8.0625 / 128, 0.25]
    out = R.labels_ref([[1, 0.5, 0.5, 0.0, 0.2], [1, 0.5, 0.5, 0.2, -0.1], [0, 0, 0, 0, 0], [1, 0.5, 0.5, 0.25, 0.125]], 128, 128, prog)
    assert not out[:3].any() and out[3].tolist() == [1, 0.5, 0.5, 0.25, 0.125]   # w <= 0 or h <= 0: zero rows, the others stay in place


def test_labels_inactive_passes_rows_through_bitwise():
    prog = R.program(100, 100, active=False, theta=0.3, tx=0.2)
    rows = np.array([[1, 0.95, 0.5, 0.3, 0.2], [0, 0, 0, 0, 0], [2, 0.1, 0.1, -1.0, 0.5], [4, 1 / 3, 2 / 3, 0.1, 0.1]])
    out = R.labels_ref(rows, 100, 100, prog)
    assert np.array_equal(out.view(np.int64), rows.view(np.int64))                 # a box that sticks out is not clipped


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
def test_sampler_is_deterministic_and_leaves_the_other_streams_alone():
    shapes = [(48, 64), (33, 47), (480, 640), (7, 1)] * 4
    seeds = list(range(100, 116))
    params, extras = aug.sample_params(seeds, shapes=shapes), aug.sample_extra(seeds, shapes)
    a, b = affine.sample_affine(seeds, shapes), affine.sample_affine(seeds, shapes)
    assert all(x["active"] == y["active"] and np.array_equal(x["fwd"], y["fwd"]) and np.array_equal(x["inv"], y["inv"])
               for x, y in zip(a, b))
    assert np.array_equal(aug.sample_params(seeds, shapes=shapes), params) and aug.sample_extra(seeds, shapes) == extras
    assert len({x["fwd"].tobytes() for x in a}) == 16
    never, always = affine.sample_affine(seeds, shapes, p=0.0), affine.sample_affine(seeds, shapes, p=1.0)
    assert [x["active"] for x in never] == [0] * 16 and [x["active"] for x in always] == [1] * 16
    assert 0 < sum(x["active"] for x in a) < 16
    for x, lo, hi in zip(a, never, always):                                        # the stream position does not depend on the outcome
        for key in ("rotate", "scale", "shear", "tx", "ty"):
            assert x[key] == lo[key] == hi[key]
        assert np.array_equal(x["fwd"], lo["fwd"]) and np.array_equal(x["inv"], hi["inv"])
    for x in a:
        assert -10 <= x["rotate"] <= 10 and 0.9 <= x["scale"] <= 1.1 and -5 <= x["shear"] <= 5
        assert -0.1 <= x["tx"] <= 0.1 and -0.1 <= x["ty"] <= 0.1 and x["shape"] in shapes
    wide = affine.sample_affine(seeds, shapes, rotate=(30, 45), scale=(1.5, 2.0), shear=(-20, -10), translate=(0.2, 0.3))
    for x in wide:
        assert 30 <= x["rotate"] <= 45 and 1.5 <= x["scale"] <= 2.0 and -20 <= x["shear"] <= -10 and 0.2 <= x["tx"] <= 0.3
    # the draws, restated: six uniforms in the order u, theta, s, phi, tx, ty from RandomState([seed, "Affi"])
    rng = np.random.RandomState([100, 0x41666669])
    u = rng.random_sample()
    drawn = [rng.uniform(-10, 10), rng.uniform(0.9, 1.1), rng.uniform(-5, 5), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)]
    assert [a[0][k] for k in ("rotate", "scale", "shear", "tx", "ty")] == drawn and a[0]["active"] == int(u < 0.5)


def test_sampler_refuses_bad_ranges():
    for kw in (dict(scale=(0, 1)), dict(scale=(-1, 1)), dict(rotate=(5, -5)), dict(p=1.5), dict(translate=(0, float("nan")))):
        with pytest.raises(ValueError):
            affine.sample_affine([1], [(4, 4)], **kw)
    with pytest.raises(ValueError):
        affine.sample_affine([1, 2], [(4, 4)])
    with pytest.raises(TypeError):
        affine.sample_affine([1], [(4, 4)], zoom=(1, 2))


def test_check_affine_programs():
    good = affine.sample_affine([1, 2], [(4, 6), (5, 5)], p=1.0)
    affine.check_affine_programs(good, [(4, 6), (5, 5)])

    def broken(**kw):
        return [dict(good[0], **kw), good[1]]
    nan = good[0]["inv"].copy()
    nan[4] = np.nan
    inf = good[0]["fwd"].copy()
    inf[2] = np.inf
    for bad, shapes in ((broken(inv=nan), [(4, 6), (5, 5)]), (broken(fwd=inf), [(4, 6), (5, 5)]), (broken(active=2), [(4, 6), (5, 5)]),
                        (broken(fwd=good[0]["fwd"][:5]), [(4, 6), (5, 5)]), (good, [(6, 4), (5, 5)]), (broken(shape=(0, 6)), [(0, 6), (5, 5)])):
        with pytest.raises(_ffi.Yv3Error) as e:
            affine.check_affine_programs(bad, shapes)
        assert e.value.code == _ffi.EINVAL
    with pytest.raises(ValueError):
        affine.check_affine_programs(good, [(4, 6)])


# ---- the C interface -----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_ffi_binds_the_entry_points():
    header = open(os.path.join(REPO, "include", "yv3.h")).read()
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("yv3_affine_augment", "yv3_affine_labels"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _ffi.EXPORTS and hasattr(handle, name)
    assert len(_ffi._SIGNATURES["yv3_affine_augment"][1]) == 11 and len(_ffi._SIGNATURES["yv3_affine_labels"][1]) == 8
    lib = _ffi.lib()
    assert lib.yv3_affine_augment(None, 1, None, None, None, 1, None, 1, None, None, None) == _ffi.EINVAL     # before any launch
    assert lib.yv3_affine_labels(None, 1, 1, None, None, None, None, None) == _ffi.EINVAL


def test_program_layout_matches_the_c_header(tmp_path):
    """yv3_affine_program as ctypes and numpy see it == as a C compiler sees include/yv3.h."""
    assert ctypes.sizeof(_ffi.AffineProgram) == 104 == affine.PROGRAM.itemsize
    names = ["active", "reserved", "fwd", "inv"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv3.h"\nint main(void){\n'
                   'printf("%zu ", sizeof(yv3_affine_program));\n'
                   + "".join('printf("%%zu ", offsetof(yv3_affine_program, %s));\n' % f for f in names) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    nums = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums == [104] + [affine.PROGRAM.fields[f][1] for f in names]
    assert nums[1:] == [getattr(_ffi.AffineProgram, f).offset for f in names]
    prog = affine.sample_affine([5], [(48, 64)], p=1.0)[0]
    packed = affine.pack_programs([prog])[0]
    assert packed["active"] == 1 and packed["reserved"] == 0
    assert np.array_equal(packed["fwd"], prog["fwd"]) and np.array_equal(packed["inv"], prog["inv"])


def test_train_batches_affine_switch_on_the_host(tmp_path):
    """The switch's host side: programs are drawn per batch from the schedule's seeds and the sources' shapes, no other draw
    moves, and the state dict's config changes only when the switch is on."""
    (tmp_path / "images").mkdir()
    paths = []
    for i in range(5):
        p = str(tmp_path / "images" / ("a%d.jpg" % i))
        Image.fromarray(np.full((6 + i, 9, 3), 40 * i, dtype=np.uint8)).save(p, format="PNG")
        paths.append(p)
    lst = tmp_path / "train.txt"
    lst.write_text("\n".join(paths) + "\n")
    off, none, default, on, custom = (aug.TrainBatches(str(lst), 2, (64, 64), seed=3, **kw) for kw in (
        dict(affine=False), dict(affine=None), {}, dict(affine=True), dict(affine=dict(rotate=(-30, 30), p=1.0))))
    assert off.state_dict() == none.state_dict() == default.state_dict() and "affine" not in off.state_dict()["config"]
    assert on.state_dict()["config"]["affine"] is True
    assert custom.state_dict()["config"]["affine"] == {"rotate": [-30.0, 30.0], "p": 1.0}
    on.load_state_dict(on.state_dict())
    off.load_state_dict(default.state_dict())
    for a, b in ((off, on), (on, off), (on, custom)):
        with pytest.raises(ValueError):
            a.load_state_dict(b.state_dict())
    with pytest.raises(ValueError):
        aug.TrainBatches(str(lst), 2, (64, 64), seed=3, affine=dict(scale=(0, 1)))
    order, seeds, _ = aug.epoch_schedule(3, 0, 5, 2)
    batches, plain, wide = list(on._host_batches()), list(default._host_batches()), list(custom._host_batches())
    assert [b[6] for b in plain] == [None] * 3
    for k, (b, b0, bw) in enumerate(zip(batches, plain, wide)):
        shapes = [im.shape[:2] for im in b[1]]
        want = affine.sample_affine(seeds[2 * k:2 * k + 2], shapes)
        assert [(p["active"], p["shape"], p["fwd"].tolist(), p["inv"].tolist()) for p in b[6]] == \
               [(p["active"], p["shape"], p["fwd"].tolist(), p["inv"].tolist()) for p in want]
        assert all(p["active"] == 1 and -30 <= p["rotate"] <= 30 for p in bw[6])
        assert np.array_equal(b[3], b0[3]) and b[0] == b0[0] and b[5] is None      # the other draws do not move
    assert len(list(on.host_batches())[0]) == 4
