"""yv3_conv2d's kernel selection against the recorded table (tests/golden/conv_select_256cu.json): the form and the number of launches of
every layer of the network at 416 and 608, six batch sizes, under every option and tune code that moves a selection rule, plus the
error code of every invalid descriptor of the error-contract test.  Host only: the two queries launch nothing."""
import json
import os

from yolo_v3_amd import _ffi
from tests import conv_select_grid as grid


def test_conv_selection_matches_the_recorded_table(golden_dir):
    with open(os.path.join(golden_dir, "conv_select_256cu.json")) as f:
        want = json.load(f)
    got = grid.table(_ffi.lib())
    assert got["cus"] == want["cus"]
    assert sorted(got["layers"]) == sorted(want["layers"]) and sorted(got["errors"]) == sorted(want["errors"])
    diff = []
    for key in sorted(want["layers"]):
        g, w = got["layers"][key].split(), want["layers"][key].split()
        assert len(g) == len(w) == 75
        diff += ["%s layer %d: form/launches %s, recorded %s" % (key, i, a, b) for i, (a, b) in enumerate(zip(g, w)) if a != b]
    diff += ["%s: %s, recorded %s" % (key, got["errors"][key], w) for key, w in sorted(want["errors"].items()) if got["errors"][key] != w]
    assert not diff, "%d differences, first:\n%s" % (len(diff), "\n".join(diff[:20]))
