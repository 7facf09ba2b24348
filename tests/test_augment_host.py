"""CPU checks of the training augmentation's restatement (tests/augment_ref.py) and sampler (yolo_v3_amd/augment.py) against the
reference's own code (tests/golden/augment.npz, written by tools/make_golden_augment.py) and hand-checked values."""
import os

import numpy as np
import pytest

from tests import augment_ref as A
from yolo_v3_amd import _ffi
from yolo_v3_amd import augment as aug

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("tag", ["darknet", "wide"])
def test_colour_draws_are_the_references(gold, tag):
    hue, sat, exp = gold["hsv_%s_settings" % tag]
    seeds = gold["hsv_seeds"]
    p = aug.sample_params(seeds, hue=hue, saturation=sat, exposure=exp, shapes=[(480, 640)] * len(seeds))
    assert np.array_equal(p[:, :3], gold["hsv_" + tag])


def test_box_conversions_are_the_references(gold):
    lab = gold["conv_labels"]
    for (W, H), a, b in zip(gold["conv_dims"], gold["conv_abs"], gold["conv_back"]):
        got = A.cxcywh_rel_to_xyxy_abs(lab, int(W), int(H))
        assert np.array_equal(got, a)
        assert np.array_equal(A.xyxy_abs_to_cxcywh_rel(a, int(W), int(H)), b)


def test_clip_and_keep_are_the_references(gold):
    for (h, w), keep, clipped in zip(gold["clip_shapes"], gold["clip_keep"], gold["clip_out"]):
        for box, k, c in zip(gold["clip_boxes"], keep, clipped):
            got_k, got_c, _ = A.clip_keep(*(float(v) for v in box), int(w), int(h))
            assert bool(got_k) == bool(k), (box, h, w)
            if k:
                assert np.array_equal(np.array(got_c), c)


@pytest.mark.parametrize("n", [0, 3, 90, 130])
def test_label_padding_is_the_references(gold, n):
    rows_in, ref = gold["fill_%d_in" % n], gold["fill_%d_out" % n]
    # identity geometry: a 100 x 100 source on a 100 x 100 canvas, no crop, no flip -> the rows come back (up to rounding)
    rows = np.zeros((n, 5))
    rows[:, 0] = rows_in[:, 0]
    rows[:, 1:3] = 0.5
    rows[:, 3:5] = 0.25
    out = A.augment_labels(rows, 100, 100, [0, 1, 1, 0, 0, 0, 0, 0], (100, 100))
    assert out.shape == ref.shape
    k = min(n, 90)
    assert np.array_equal(out[:k, 0], rows_in[:k, 0])
    assert np.array_equal(ref[:k], rows_in[:k].astype(np.float32)) and not ref[k:].any()
    assert not out[k:].any()
    assert np.allclose(out[:k, 1:], [0.5, 0.5, 0.25, 0.25], atol=1e-12)


# ---- colour conversions, hand-checked -----------------------------------------------------------------------------------------
def px(*rgb):
    return np.array(rgb, dtype=np.uint8).reshape(1, 1, 3)


@pytest.mark.parametrize("rgb,hsv", [((255, 0, 0), (0, 255, 255)), ((0, 255, 0), (60, 255, 255)), ((0, 0, 255), (120, 255, 255)),
                                     ((255, 255, 0), (30, 255, 255)), ((0, 255, 255), (90, 255, 255)), ((255, 0, 255), (150, 255, 255)),
                                     ((128, 128, 128), (0, 0, 128)), ((0, 0, 0), (0, 0, 0)), ((255, 255, 255), (0, 0, 255)),
                                     ((200, 100, 50), (10, 191, 200))])
def test_rgb2hsv_hand_checked(rgb, hsv):
    assert tuple(A.rgb2hsv_u8(px(*rgb))[0, 0]) == hsv


@pytest.mark.parametrize("hsv,rgb", [((0, 255, 255), (255, 0, 0)), ((60, 255, 255), (0, 255, 0)), ((120, 255, 255), (0, 0, 255)),
                                     ((37, 0, 200), (200, 200, 200)), ((0, 0, 0), (0, 0, 0)),
                                     ((180, 255, 255), (255, 0, 0)),         # 180 wraps to 0
                                     ((255, 255, 255), (0, 255, 128)),       # 255 * 6/180 = 8.5 -> 2.5: sector 2, half-way
                                     ((179, 255, 255), (255, 0, 8))])        # sector 5, 1 - 0.9666667 -> 8.5 - 1 ulp
def test_hsv2rgb_hand_checked(hsv, rgb):
    assert tuple(A.hsv2rgb_u8(px(*hsv))[0, 0]) == rgb


def test_hue_shift_clips_below_zero_and_wraps_above_179():
    red, green = px(255, 0, 0), px(0, 255, 0)
    assert tuple(A.hsv_jitter(red, -17.9, 1.0, 1.0)[0, 0]) == (255, 0, 0)          # 0 - 17.9 clips to 0: red stays red
    assert tuple(A.hsv_jitter(green, -17.9, 1.0, 1.0)[0, 0]) == tuple(A.hsv2rgb_u8(px(42, 255, 255))[0, 0])
    assert tuple(A.hsv_jitter(px(0, 0, 255), 17.9 * 4, 1.0, 1.0)[0, 0]) == tuple(A.hsv2rgb_u8(px(191, 255, 255))[0, 0])
    assert tuple(A.hsv2rgb_u8(px(191, 255, 255))[0, 0]) == tuple(A.hsv2rgb_u8(px(11, 255, 255))[0, 0])   # 191 wraps to 11


def test_saturation_and_exposure_truncate_and_clip():
    img = px(200, 100, 50)                                                          # hsv (10, 191, 200)
    h, s, v = A.rgb2hsv_u8(A.hsv_jitter(img, 0.0, 1.5, 1.5))[0, 0]
    assert (s, v) == (255, 255)                                                     # 286.5 / 300 clip
    h, s, v = A.rgb2hsv_u8(A.hsv_jitter(img, 0.0, 1 / 1.5, 1 / 1.5))[0, 0]
    assert abs(int(s) - 127) <= 1 and abs(int(v) - 133) <= 1                        # 127.33, 133.33 truncated (+ round trip)


def test_roundtrip_is_not_identity_everywhere_but_close():
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (40, 50, 3)).astype(np.uint8)
    rt = A.hsv_roundtrip(img)
    assert np.abs(rt.astype(int) - img.astype(int)).max() <= 8
    assert not np.array_equal(rt, img)                                             # the 8-bit round trip loses bits


def test_crop_pad_flip_layout():
    img = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3)
    out = A.crop_pad_flip(img, 1, -2, -1, 2, 0)                                     # top pads 1, right crops 2, bottom crops 1, left pads 2
    assert out.shape == (4, 5, 3)
    assert (out[0] == 128).all() and (out[:, :2] == 128).all()
    assert np.array_equal(out[1:, 2:], img[:3, :3])
    f = A.crop_pad_flip(img, 1, -2, -1, 2, 1)
    assert np.array_equal(f, out[:, ::-1])
    everything = A.crop_pad_flip(img, -3, -4, 0, 0, 0)
    assert np.array_equal(everything, img[3:, :1])


# ---- sampler ------------------------------------------------------------------------------------------------------------------
def test_sampler_bounds_and_determinism():
    shapes = [(480, 640), (1, 1), (97, 1231), (333, 500), (2, 3), (3, 2)] * 50
    seeds = np.arange(len(shapes)) * 7919 + 3
    p = aug.sample_params(seeds, shapes=shapes)
    assert p.shape == (len(shapes), 8) and p.dtype == np.float64
    assert np.array_equal(p, aug.sample_params(seeds, shapes=shapes))
    assert not np.array_equal(p, aug.sample_params(seeds + 1, shapes=shapes))
    assert (np.abs(p[:, 0]) <= 0.1 * 179).all()
    for k in (1, 2):
        assert ((p[:, k] >= 1 / 1.5) & (p[:, k] <= 1.5)).all()
        assert (p[:, k] < 1).any() and (p[:, k] > 1).any()
    H = np.array([s[0] for s in shapes], dtype=np.float64)
    W = np.array([s[1] for s in shapes], dtype=np.float64)
    for k, n in ((3, H), (4, W), (5, H), (6, W)):
        assert np.array_equal(p[:, k], np.rint(p[:, k]))
        assert (np.abs(p[:, k]) <= np.rint(0.3 * n)).all()
    assert (H + p[:, 3] + p[:, 5] >= 1).all() and (W + p[:, 6] + p[:, 4] >= 1).all()
    assert set(np.unique(p[:, 7])) == {0.0, 1.0}
    aug.check_params(p, shapes, (416, 416))                                         # every draw is a valid parameter row


def test_keep_one_pixel():
    assert aug.keep_one_pixel(-1.0, -1.0, 2) == (0.0, -1.0)
    assert aug.keep_one_pixel(-1.0, -2.0, 3) == (-1.0, -1.0)
    assert aug.keep_one_pixel(-1.0, 1.0, 1) == (-1.0, 1.0)


def test_sampler_stream_is_documented():
    p = aug.sample_params([11], hue=0.2, saturation=2.0, exposure=1.25, jitter=0.25, flip=0.5, shapes=[(100, 200)])[0]
    r = np.random.RandomState(11)
    dhue = r.uniform(-0.2, 0.2) * 179
    dsat = r.uniform(1, 2.0)
    dsat = 1 / dsat if r.random_sample() < 0.5 else dsat
    dexp = r.uniform(1, 1.25)
    dexp = 1 / dexp if r.random_sample() < 0.5 else dexp
    sides = [np.rint(r.uniform(-0.25, 0.25) * n) for n in (100, 200, 100, 200)]
    flip = 1.0 if r.random_sample() < 0.5 else 0.0
    assert np.array_equal(p, [dhue, dsat, dexp] + sides + [flip])


@pytest.mark.parametrize("row,code", [([np.nan, 1, 1, 0, 0, 0, 0, 0], _ffi.EINVAL), ([0, np.inf, 1, 0, 0, 0, 0, 0], _ffi.EINVAL),
                                      ([0, 1, -0.5, 0, 0, 0, 0, 0], _ffi.EINVAL), ([0, 1, 1, 0.5, 0, 0, 0, 0], _ffi.EINVAL),
                                      ([0, 1, 1, 0, 0, 0, 0, 2], _ffi.EINVAL), ([0, 1, 1, -6, 0, -4, 0, 0], _ffi.ESHAPE),
                                      ([0, 1, 1, 0, -3, 0, -7, 0], _ffi.ESHAPE), ([0, 1, 1, 0, 0, 0, 0, 0], 0)])
def test_check_params_codes(row, code):
    if code == 0:
        aug.check_params(np.array([row], dtype=np.float64), [(10, 10)], (416, 416))
        return
    with pytest.raises(_ffi.Yv3Error) as e:
        aug.check_params(np.array([row], dtype=np.float64), [(10, 10)], (416, 416))
    assert e.value.code == code


def test_label_restatement_geometry():
    # one box in the middle of a 100 x 200 (H x W) source, padded left by 20 and flipped, letterboxed to 416
    p = [0, 1, 1, 0, 0, 0, 20, 1]
    out = A.augment_labels([[3, 0.5, 0.5, 0.2, 0.4]], 100, 200, p, (416, 416))
    W1 = 220
    x1, x2 = 80 + 20, 120 + 20
    x1, x2 = (W1 - 1) - x2, (W1 - 1) - x1
    rw, rh, xp, yp = 416, int(100 * 416 / 220), 0, (416 - int(100 * 416 / 220)) // 2
    x1, x2 = x1 * rw / W1 + xp, x2 * rw / W1 + xp
    y1, y2 = 30 * rh / 100 + yp, 70 * rh / 100 + yp
    assert np.allclose(out[0], [3, (x1 + x2) / 2 / 416, (y1 + y2) / 2 / 416, (x2 - x1) / 416, (y2 - y1) / 416], atol=1e-12)
    assert not out[1:].any()
