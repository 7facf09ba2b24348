"""yv3_conv2d's kernel selection against the recorded table (tests/golden/conv_select_256cu.json): the form, the number of launches and the
whole choice (yv3_conv2d_kernel: kernel, tiles, loop, schedule, grids) of every layer of the network at 416 and 608, six batch sizes, under
every option and tune code that moves a selection rule, plus the error code of every invalid descriptor of the error-contract test.
Host only: the three queries launch nothing."""
import json
import os

from yolo_v3_amd import _ffi
from tests import conv_select_grid as grid


def test_conv_selection_matches_the_recorded_table(golden_dir):
    with open(os.path.join(golden_dir, "conv_select_256cu.json")) as f:
        want = json.load(f)
    rows, errors = grid.answers(_ffi.lib())
    assert want["cus"] == 256
    assert sorted(rows) == sorted(want["layers"]) and sorted(errors) == sorted(want["errors"])
    for size in grid.SIZES:
        distinct, layer_of = grid.classes(size)
        assert want["layer_of"][str(size)].split() == [str(i) for i in layer_of] and len(layer_of) == 75
    diff = []
    for key in sorted(want["layers"]):
        g, w = rows[key], [grid.parse(t, want["kernels"]) for t in want["layers"][key].split()]
        assert len(g) == len(w) == len(grid.classes(int(key.split("/")[1]))[0])
        diff += ["%s distinct layer %d: form, launches, kernel %s, recorded %s" % (key, i, a, b) for i, (a, b) in enumerate(zip(g, w)) if a != b]
    diff += ["%s: %s, recorded %s" % (key, errors[key], grid.parse(w, want["kernels"])) for key, w in sorted(want["errors"].items())
             if errors[key] != grid.parse(w, want["kernels"])]
    assert not diff, "%d differences, first:\n%s" % (len(diff), "\n".join(diff[:20]))


def test_kernel_query_buffer_contract():
    """yv3_conv2d_kernel: a line of at most 96 bytes with its NUL; YV3_EINVAL for a buffer it does not fit, the launch's code for a bad descriptor."""
    import ctypes
    lib = _ffi.lib()
    d = grid.make_desc(lib, "f32", 416, 8, grid.classes(416)[0][5])
    line = _ffi.conv2d_kernel(d)
    assert 0 < len(line) < _ffi.KERNEL_LINE_BYTES
    exact = ctypes.create_string_buffer(len(line) + 1)
    assert lib.yv3_conv2d_kernel(ctypes.byref(d), exact, len(exact)) == 0 and exact.value.decode() == line
    short = ctypes.create_string_buffer(len(line))
    assert lib.yv3_conv2d_kernel(ctypes.byref(d), short, len(short)) == _ffi.EINVAL
    assert lib.yv3_conv2d_kernel(ctypes.byref(d), None, 0) == _ffi.EINVAL
    d.k = 2
    assert lib.yv3_conv2d_kernel(ctypes.byref(d), exact, len(exact)) == lib.yv3_conv2d_form(ctypes.byref(d)) == _ffi.ESHAPE
