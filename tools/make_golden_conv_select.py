"""Records tests/golden/conv_select_256cu.json: yv3_conv2d_form / yv3_conv2d_launches / yv3_conv2d_kernel over the grid of
tests/conv_select_grid.py.  The kernel lines already in the file keep their index, new ones are appended: a changed rule shows up as the
tokens it moved.  With --wide-heads: tests/golden/conv_select_wide_heads.json instead, the same three answers for the head convolution of
networks with more than 80 classes (conv_select_grid.wide_heads_table), in every math mode.

Runs on the host (nothing is launched; without a GPU the library counts 256 compute units).  The table pins the library's kernel-selection
rules: regenerate it only together with a deliberate change of a rule, and say which rows moved.

    python tools/make_golden_conv_select.py [--wide-heads] [--out FILE]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from yolo_v3_amd import _ffi                      # noqa: E402
from tests import conv_select_grid as grid        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide-heads", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "tests", "golden", "conv_select_wide_heads.json" if args.wide_heads else "conv_select_256cu.json")
    old = []
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f).get("kernels", [])
    table = grid.wide_heads_table(_ffi.lib(), old) if args.wide_heads else grid.table(_ffi.lib(), old)
    with open(args.out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    if args.wide_heads:
        print("%s: %d head rows, %d kernel lines (%d new)" % (args.out, len(table["heads"]), len(table["kernels"]), len(table["kernels"]) - len(old)))
        return
    print("%s: %d layer rows, %d invalid descriptors, %d kernel lines (%d new)"
          % (args.out, len(table["layers"]), len(table["errors"]), len(table["kernels"]), len(table["kernels"]) - len(old)))


if __name__ == "__main__":
    main()
