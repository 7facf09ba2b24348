"""Static description of the YOLOv3 / Darknet-53 convolution stack.

Two tables drive everything that needs to agree on the network.  ``conv_specs``:
layer order and shapes -- the darknet ``.weights`` stream order (reference
``darknet.py:292-303`` walks the module tree depth-first, which equals the darknet
cfg order), the synthetic weight generator, the parameter containers in
``darknet.py``.  ``wiring``: which convolution reads, upsamples, concatenates and
adds which output, and which three are heads -- the HIP execution plan and the I8
scale folding in ``engine.py``, the training graph in ``backprop.py`` and the
layer geometry (``conv_hw``) all read it; nothing else in the package walks the
architecture.

Reference architecture: ``darknet.py:72-81`` (backbone ``Darknet([1,2,8,8,4])``),
``darknet.py:107-120`` (``PreDetectionConvGroup``), ``darknet.py:153-162``
(``UpsampleGroup``), wiring ``darknet.py:179-194``.
"""
from collections import namedtuple

# name  : state_dict prefix of the module that owns the convolution
# bn    : True  -> conv(no bias) + BatchNorm(eval) + LeakyReLU(0.1)   (reference conv_bn_relu)
#         False -> plain conv with bias, no activation                 (the three head convs)
# res2  : True for the second conv of a res_layer (used by the synthetic weight recipe)
ConvSpec = namedtuple("ConvSpec", "name cin cout k stride bn res2")

BACKBONE_BLOCKS = (1, 2, 8, 8, 4)
DEFAULT_ANCHORS = (10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326)
ANCHOR_MASKS = ((6, 7, 8), (3, 4, 5), (0, 1, 2))


def backbone_specs(blocks=BACKBONE_BLOCKS, nout=32):
    """52 convolutions of the Darknet-53 feature extractor, cfg order."""
    specs = [ConvSpec("feature.mlist.0", 3, nout, 3, 1, True, False)]
    idx = 1
    for stage, nblk in enumerate(blocks):
        cin = nout * (2 ** stage)
        specs.append(ConvSpec("feature.mlist.%d" % idx, cin, cin * 2, 3, 2, True, False))
        idx += 1
        for _ in range(nblk):
            c = cin * 2
            specs.append(ConvSpec("feature.mlist.%d.conv1" % idx, c, c // 2, 1, 1, True, False))
            specs.append(ConvSpec("feature.mlist.%d.conv2" % idx, c // 2, c, 3, 1, True, True))
            idx += 1
    return specs


def predet_specs(prefix, nin, nout, num_class):
    """7 convolutions of one detection branch: (1x1 n, 3x3 2n) x3 then plain 1x1 -> 3*(5+C)."""
    specs = []
    cin = nin
    for i in range(3):
        specs.append(ConvSpec("%s.mlist.%d" % (prefix, 2 * i), cin, nout, 1, 1, True, False))
        specs.append(ConvSpec("%s.mlist.%d" % (prefix, 2 * i + 1), nout, nout * 2, 3, 1, True, False))
        cin = nout * 2
    specs.append(ConvSpec("%s.mlist.6" % prefix, cin, (num_class + 5) * 3, 1, 1, False, False))
    return specs


def conv_specs(num_class=80):
    """All 75 convolutions in darknet ``.weights`` stream order."""
    s = backbone_specs()
    s += predet_specs("pre_det1", 1024, 512, num_class)
    s.append(ConvSpec("up1.conv", 512, 256, 1, 1, True, False))
    s += predet_specs("pre_det2", 768, 256, num_class)
    s.append(ConvSpec("up2.conv", 256, 128, 1, 1, True, False))
    s += predet_specs("pre_det3", 384, 128, num_class)
    return s


def floats_in_stream(specs):
    """Number of float32 values a darknet .weights stream holds for ``specs``."""
    n = 0
    for sp in specs:
        n += sp.cout * sp.cin * sp.k * sp.k
        n += 4 * sp.cout if sp.bn else sp.cout
    return n


def conv_macs_per_image(size, num_class=80):
    """Multiply-accumulates of the 75 convolutions for one ``size`` x ``size`` image."""
    total = 0
    for sp, (h, w) in zip(conv_specs(num_class), conv_output_hw(size, num_class)):
        total += h * w * sp.cout * sp.cin * sp.k * sp.k
    return total


# x        : index of the conv whose output this one reads (None: feature.mlist.0 reads the image)
# x2       : only at the two joins (pre_det2.mlist.0, pre_det3.mlist.0), which read cat(nearest_up2x(x), x2): x is the up-conv, x2 the
#            route (feature.mlist.23.conv2, feature.mlist.14.conv2); None everywhere else
# cin_up   : at a join, the channels of the upsampled part (specs[x].cout); else 0
# residual : index of the conv whose output the epilogue adds (the 23 res_layer conv2s); else None
# head     : 0 / 1 / 2 on the three plain head convs; else None
Wire = namedtuple("Wire", "x x2 cin_up residual head")
_wiring = None


def wiring(specs):
    """One Wire per convolution of ``specs`` (``conv_specs`` order): the network's wiring (reference darknet.py:72-88 backbone with
    x + conv2(conv1(x)), :107-120 detection branches, :179-194 upsample + concat).  No field depends on the class count, so the table
    is built once."""
    global _wiring
    if _wiring is None:
        wires = [Wire(None, None, 0, None, None)]

        def add(x, x2=None, residual=None, head=None):
            wires.append(Wire(x, x2, specs[x].cout if x2 is not None else 0, residual, head))
            return len(wires) - 1

        x, routes = 0, []
        for nblk in BACKBONE_BLOCKS:
            x = add(x)                                  # stride-2 3x3
            for _ in range(nblk):
                x = add(add(x), residual=x)             # x + conv2(conv1(x)), :53
            routes.append(x)
        for head, route in enumerate((None, routes[3], routes[2])):      # mlist[23] 26x26x512, mlist[14] 52x52x256 (:180-181)
            if route is not None:
                x = add(x)                              # upK.conv reads the fifth conv of the branch before (addCachedOut(-3), :185)
            x = add(x, route)
            for _ in range(4):
                x = add(x)
            add(add(x), head=head)
        assert len(wires) == len(specs) == 75
        _wiring = tuple(wires)
    return _wiring


def out_hw(h, w, k, stride):
    pad = (k - 1) // 2
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def conv_hw(H, W):
    """(h, w, ho, wo) of every conv in ``conv_specs`` order for an H x W image: the picture it reads and the one it writes.  A join
    reads at its route's size (the up-conv's output is upsampled to it)."""
    specs = conv_specs()
    geo = []
    for sp, wr in zip(specs, wiring(specs)):
        src = wr.x if wr.x2 is None else wr.x2
        h, w = (H, W) if src is None else geo[src][2:]
        geo.append((h, w) + out_hw(h, w, sp.k, sp.stride))
    return geo


def conv_output_hw(size, num_class=80):
    """Output (H, W) of every conv in ``conv_specs`` order for a square input."""
    return [g[2:] for g in conv_hw(size, size)]

