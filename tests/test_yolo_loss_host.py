"""CPU checks of the YOLO loss: the float64 restatement (tests/yolo_loss_ref.py) against the reference-produced fixture
(tests/golden/yolo_loss.npz, tools/make_golden_yolo_loss.py), the C descriptor's layout, and the host-side argument checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import yolo_loss_ref as R
from yolo_v3_amd import _ffi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "yolo_loss.npz")


def assert_components(got, want, rtol=1e-5, floor=1e-30):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.all(np.abs(got - want) <= rtol * np.abs(want) + floor), (got, want)


def assert_grad(got, want, rtol=1e-4):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    atol = 1e-6 * float(np.abs(want).max()) if want.size else 0.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("spec", R.CASES, ids=[c["name"] for c in R.CASES])
def test_restatement_matches_the_reference(gold, spec):
    n = spec["name"]
    x, tg = R.make_case(spec, int(gold[n + "/attempt"]))
    res = R.yolo_loss(x, tg, R.ANCHORS, spec["mask"], spec["img_dim"][1], spec["C"])
    assert R.margins_ok(res["margins"])
    assert [res["nCorrect"], res["nGT"]] == list(gold[n + "/counts"])
    B = spec["B"]
    vals = gold[n + "/values"]
    assert_components(res["sums"], vals[2:8] * B)          # the six components (the fixture holds item() / nB)
    assert_components(res["sums"].sum(), vals[0])
    assert_grad(res["grad"], gold[n + "/grad"])


def test_fixture_covers_the_issue_cases(gold):
    names = {c["name"]: c for c in R.CASES}
    assert {tuple(c["mask"]) for c in R.CASES} == {(0, 1, 2), (3, 4, 5), (6, 7, 8)}
    assert {c["C"] for c in R.CASES} == {2, 80}
    assert gold["hits/counts"][0] > 0 and gold["saturated/counts"][0] > 0
    assert gold["t0/counts"][1] == 0
    x, tg = R.make_case(names["quirks"], int(gold["quirks/attempt"]))
    assert (tg[1] == 0).all() and tg[0, 3].sum() == 0 and tg[0, 4].sum() > 0 and (tg[2, :, 3] == 0).any()
    x, _ = R.make_case(names["saturated"], int(gold["saturated/attempt"]))
    assert {30.0, -30.0, 120.0, -120.0} <= set(np.unique(x).tolist())
    assert os.path.getsize(GOLD) < 4 << 20


def test_yolo_loss_desc_layout_matches_the_c_header(tmp_path):
    """struct yv3_yolo_loss_desc as ctypes sees it == as a C compiler sees include/yv3.h (size and every field offset)."""
    fields = [f for f, _ in _ffi.YoloLossDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv3.h"\nint main(void){printf("%zu", sizeof(yv3_yolo_loss_desc));\n'
                   + "".join('printf(" %%zu", offsetof(yv3_yolo_loss_desc, %s));\n' % f for f in fields)
                   + 'printf(" %d", YV3_YOLO_LOSS_MAX_ROWS);\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_ffi.YoloLossDesc)] + [getattr(_ffi.YoloLossDesc, f).offset for f in fields] + [_ffi.YOLO_LOSS_MAX_ROWS]


def _valid_desc():
    """A descriptor that passes every host check; its pointers are dummies, so it is never handed over with a workspace."""
    d = _ffi.YoloLossDesc()
    d.logits = d.target = d.sums = d.counts = d.status = 4096
    d.B, d.H, d.W, d.T, d.num_class = 2, 13, 13, 4, 80
    d.stride_b, d.stride_p, d.stride_c = 13 * 13 * 255, 1, 13 * 13
    d.img_dim_h = 416.0
    for k in range(18):
        d.anchors[k] = float(R.ANCHORS[k // 2][k % 2])
    d.mask[0], d.mask[1], d.mask[2] = 6, 7, 8
    return d


def test_yolo_loss_rejects_bad_arguments_before_launching():
    lib = _ffi.lib()
    ws_need = lib.yv3_yolo_loss_workspace_bytes(2, 13, 13, 4)
    assert ws_need > 0
    assert lib.yv3_yolo_loss_workspace_bytes(0, 13, 13, 4) == 0
    assert lib.yv3_yolo_loss_workspace_bytes(2, 13, 13, -1) == 0
    assert lib.yv3_yolo_loss_workspace_bytes(2, 13, 13, 0) > 0
    # a valid descriptor only fails on the workspace size here
    assert lib.yv3_yolo_loss(_valid_desc(), 4096, ws_need - 1, None) == _ffi.EWORKSPACE
    assert lib.yv3_yolo_loss(None, 4096, ws_need, None) == _ffi.EINVAL
    assert lib.yv3_yolo_loss(_valid_desc(), None, ws_need, None) == _ffi.EINVAL
    cases = [
        ("logits", None, _ffi.EINVAL), ("sums", None, _ffi.EINVAL), ("counts", None, _ffi.EINVAL), ("status", None, _ffi.EINVAL),
        ("target", None, _ffi.EINVAL), ("B", 0, _ffi.EINVAL), ("H", -1, _ffi.EINVAL), ("T", -1, _ffi.EINVAL),
        ("num_class", 0, _ffi.EINVAL), ("img_dim_h", 0.0, _ffi.EINVAL), ("img_dim_h", float("nan"), _ffi.EINVAL),
        ("stride_c", 0, _ffi.ESHAPE), ("stride_p", 13 * 13, _ffi.ESHAPE),           # channel and pixel strides overlap
        ("stride_b", 100, _ffi.ESHAPE),
    ]
    for field, value, code in cases:
        d = _valid_desc()
        setattr(d, field, value)
        assert lib.yv3_yolo_loss(d, 4096, 1 << 40, None) == code, field
    d = _valid_desc()
    d.mask[1] = 9
    assert lib.yv3_yolo_loss(d, 4096, 1 << 40, None) == _ffi.EINVAL
    d = _valid_desc()
    d.anchors[3] = -1.0
    assert lib.yv3_yolo_loss(d, 4096, 1 << 40, None) == _ffi.EINVAL
    d = _valid_desc()
    d.T, d.target = 0, None                                   # T = 0 needs no target pointer: only the workspace check is left
    assert lib.yv3_yolo_loss(d, 4096, 0, None) == _ffi.EWORKSPACE


def test_layer_refuses_cpu_logits_with_both_error_types():
    import torch
    from yolo_v3_amd import YoloLayer
    layer = YoloLayer(R.ANCHORS, [6, 7, 8], (416, 416), 80)
    with pytest.raises(_ffi.Yv3Error) as e:
        layer(torch.zeros(1, 255, 13, 13), (416, 416), torch.zeros(1, 1, 5))
    assert isinstance(e.value, NotImplementedError)
